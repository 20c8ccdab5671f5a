"""Crafted content for the JPEG encoders' tests (numpy only, deterministic).

The encoders are checked byte for byte against libjpeg-turbo, so an input is
worth what it makes libjpeg do.  The cases here are built backwards from the
quantised coefficients the entropy coders should meet -- a Huffman tree deeper
than 16, zero runs around every ZRL rule of jcphuff.c, the largest DC and AC
categories, EOB runs in the thousands -- or are full-swing pixels for
k_jpeg_fdct.  tests/test_encoder_content_cpu.py proves on Pillow's files alone
that each case has its property and runs the host model on it;
tests/test_gpu_encoder_content.py then runs the kernels.

Coefficient blocks are (bh, bw, 64) integers; ``k`` is always the zigzag index.
"""
import functools
from collections import namedtuple

import numpy as np

from . import _adversarial as A
from ._jpeg_files import ZZ

# jcparam.c std_luminance_quant_tbl, natural order
STD_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
                     14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])

# name: the case with its mode ("deep17_420"); px: (H, W) gray or (H, W, 3);
# subsampling: 0 = 4:4:4, 2 = 4:2:0 (0 for gray); target: the zigzag luma
# blocks the pixels were built from (None: a pixel case)
Case = namedtuple("Case", "name px quality subsampling target")


def luma_table(quality):
    """jcparam.c jpeg_quality_scaling + jpeg_add_quant_table with force_baseline: natural order"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((STD_LUMA * scale + 50) // 100, 1, 255)


def zigzag_to_natural(blocks):
    nat = np.zeros(blocks.shape, np.int64)
    nat[..., ZZ] = blocks
    return nat


_U = np.arange(8)
_C = np.cos((2 * _U[None, :] + 1) * _U[:, None] * np.pi / 16) * np.where(_U == 0, np.sqrt(0.125), 0.5)[:, None]


def image_from_coefficients(blocks, quality):
    """(bh, bw, 64) natural-order quantised coefficients -> the (bh * 8, bw * 8)
    uint8 plane whose luminance blocks quantise to them at ``quality``:
    float64 IDCT of the dequantised blocks, + 128, rounded."""
    blocks = np.asarray(blocks)
    bh, bw, _ = blocks.shape
    deq = (blocks * luma_table(quality)).astype(np.float64).reshape(bh, bw, 8, 8)
    px = np.einsum("uy,...uv,vx->...yx", _C, deq, _C) + 128.0
    assert px.min() >= -0.5 and px.max() <= 255.5, f"samples {px.min():.1f} .. {px.max():.1f} would be clipped"
    return np.clip(np.rint(px), 0, 255).astype(np.uint8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _gray3(g):
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


def _modes(name, g, quality, target, modes):
    """the gray plane ``g`` as gray and as R = G = B (libjpeg's Y is then g exactly, chroma flat)"""
    out = []
    for m in modes:
        px = g if m == "gray" else _gray3(g)
        out.append(Case(f"{name}_{m}", px, quality, 2 if m == "420" else 0, target))
    return out


# ---- a Huffman tree deeper than 16 ---------------------------------------------
DEEP_SEED = 17


def deep_counts(nclasses, nblocks):
    """1, 2, 3, 5, 8 ...: each count the sum of the two before it, so every
    merge of jpeg_gen_optimal_table takes the tree so far and the next symbol
    (starting 1, 1 would tie with the reserved symbol and fork the chain); the
    last class takes the blocks that are left."""
    c = [1, 2]
    while len(c) < nclasses - 1:
        c.append(c[-1] + c[-2])
    last = nblocks - sum(c)
    assert last >= c[-1] + c[-2], "the grid is too small to keep the chain"
    return c + [last]


def deep_classes(nclasses):
    """(k, nb): one coefficient at zigzag k whose value has nb bits in the
    1-5 / Al=2 scan -- nb-major, k-minor"""
    return [(1 + i % 5, 1 + i // 5) for i in range(nclasses)]


@functools.lru_cache(None)
def deep_blocks(nclasses, side):
    """side x side zigzag blocks, each with one coefficient 4 * 2^(nb-1) + 1 at k in 1..5"""
    n = side * side
    cls = np.repeat(np.arange(nclasses), deep_counts(nclasses, n))
    cls = cls[np.random.default_rng(DEEP_SEED).permutation(n)]
    b = np.zeros((n, 64), np.int64)
    for i, (k, nb) in enumerate(deep_classes(nclasses)):
        b[cls == i, k] = 4 * 2 ** (nb - 1) + 1
    return b.reshape(side, side, 64)


def deep17():
    """16 classes + EOB + the reserved symbol: natural depth 17.  66 x 66 blocks."""
    t = deep_blocks(16, 66)
    return _modes("deep17", image_from_coefficients(zigzag_to_natural(t), 50), 50, t, ("gray", "444", "420"))


def deep18():
    """17 classes: natural depth 18.  84 x 84 blocks."""
    t = deep_blocks(17, 84)
    return _modes("deep18", image_from_coefficients(zigzag_to_natural(t), 50), 50, t, ("gray",))


# ---- zero runs -----------------------------------------------------------------
# Quality 75, not 50: |v| = 8 at k = 60 dequantises to 800 at quality 50, a
# sample swing of +-200 that no 8-bit block holds; at 75 (steps 5 .. 61) it is
# +-100.  The CPU test shows that libjpeg still quantises to the targets exactly.
ZERO_RUNS_QUALITY = 75
ZERO_RUNS_ROWS = (
    # a single coefficient around every multiple of 16, and the last one
    [{k: 4 if i % 2 else -4} for i, k in enumerate((15, 16, 17, 31, 32, 33, 47, 48, 49, 63))]
    + [{1: -4, 63: 4}, {1: 5, 63: -6}]
    # first nonzero behind a run longer than 15 in: the 6-63 Al=2 scan (|v| >= 4), the Ah=2 scan
    # (2..3), the last scan (1)
    + [{40: 4}, {40: -5}, {40: 2}, {40: -3}, {40: 1}, {40: -1}]
    # a correction bit (k = 1), 38 zeros, newly nonzero at k = 40 in the Ah=2 scan: two ZRLs, the
    # correction bit behind the first
    + [{1: 9, 40: -2}, {1: -10, 40: 2}, {1: -11, 40: 3}]
    # newly nonzero at k = 3, then 56 zeros and a correction bit at k = 60: no ZRL, the bit joins the EOB run
    + [{3: 2, 60: -8}, {3: -2, 60: 8}, {3: 3, 60: 9}]
)


@functools.lru_cache(None)
def zero_runs_blocks():
    """6 x 8 blocks: ZERO_RUNS_ROWS twice over"""
    b = np.zeros((48, 64), np.int64)
    for i in range(48):
        for k, v in ZERO_RUNS_ROWS[i % len(ZERO_RUNS_ROWS)].items():
            b[i, k] = v
    return b.reshape(6, 8, 64)


def zero_runs():
    t = zero_runs_blocks()
    q = ZERO_RUNS_QUALITY
    return _modes("zero_runs", image_from_coefficients(zigzag_to_natural(t), q), q, t, ("gray", "444"))


def baseline_zrls(blocks):
    """ZRL symbols of the sequential coding of zigzag blocks: a run of r zeros
    before a nonzero coefficient takes r // 16 of them; trailing zeros none"""
    n = 0
    for blk in np.asarray(blocks).reshape(-1, 64):
        nzk = np.flatnonzero(blk[1:]) + 1
        prev = 0
        for k in nzk:
            n += (k - prev - 1) // 16
            prev = k
    return n


# ---- full-swing pixels ---------------------------------------------------------
def dc_swing():
    """8 x 8-px blocks of flat 0 and flat 255 in a checker: at quality 100 the
    DCs are -1024 and 1016, every difference inside a row +-2040"""
    g = (A._checker_plane(64, 48, 8) * 255).astype(np.uint8)
    return _modes("dc_swing", g, 100, None, ("gray", "444", "420"))


def ac_max():
    """Block i (natural order, 1..63) is 255 where AC basis function i is
    positive and 0 elsewhere -- the 8-bit block with the largest coefficient
    i; block 0 is flat 128."""
    g = np.full((64, 64), 128, np.uint8)
    for i in range(1, 64):
        basis = _C[i // 8][:, None] * _C[i % 8][None, :]
        g[(i // 8) * 8:(i // 8) * 8 + 8, (i % 8) * 8:(i % 8) * 8 + 8] = np.where(basis > 0, 255, 0)
    return _modes("ac_max", g, 100, None, ("gray", "444"))


def binary_noise():
    px = (np.random.default_rng(100).integers(0, 2, (64, 64, 3)) * 255).astype(np.uint8)
    return [Case("binary_noise_gray", np.ascontiguousarray(px[..., 1]), 100, 0, None),
            Case("binary_noise_444", px, 100, 0, None), Case("binary_noise_420", px, 100, 2, None)]


# ---- EOB runs in the thousands -------------------------------------------------
LONG_EOB_W = 65500  # libjpeg's widest image: 8188 blocks in one restart interval


@functools.lru_cache(None)
def long_eob_blocks(single):
    t = np.zeros((1, (LONG_EOB_W + 7) // 8, 64), np.int64)
    if single:
        t[0, t.shape[1] // 2, 1] = 5
    return t


def long_eob():
    """flat 128: every AC scan is one EOB run of 8188 (0xC0, 12 extra bits);
    with one coefficient at k = 1 of the middle block, runs of 4094 (0xB0, 11
    bits) and 4093 on its sides in the scans that code it"""
    out = []
    for name, single in (("long_eob_flat", False), ("long_eob_single", True)):
        t = long_eob_blocks(single)
        px = image_from_coefficients(zigzag_to_natural(t), 50)
        assert not t[0, -1].any()  # the block the width cuts is flat: libjpeg's edge padding gives it back
        out.append(Case(name, np.ascontiguousarray(px[:, :LONG_EOB_W]), 50, 0, t))
    return out


# ---- the pixel corpus of tests/_adversarial.py ------------------------------------
PIXEL_SIZES = ((61, 37), (48, 32))
PIXEL_QUALITIES = (1, 50, 100)


def pixel_contents(W, H):
    out = [(f"checker{b}", A.checker(W, H, b)) for b in (1, 3, 8)]
    out += [("stripes", A.stripes(W, H)), ("impulses", A.impulses(W, H)),
            ("impulses_inv", A.impulses(W, H, inverse=True)), ("noise", A.noise(W, H, W + H))]
    return out + [(f"flat{v}", A.flat(W, H, v)) for v in A.FLAT_VALUES]


@functools.lru_cache(None)
def pixel_corpus(quality):
    """every content x size x mode at one quality (gray: the G plane)"""
    out = []
    for W, H in PIXEL_SIZES:
        for name, px in pixel_contents(W, H):
            n = f"{name}_{W}x{H}_q{quality}"
            out += [Case(f"{n}_444", px, quality, 0, None), Case(f"{n}_420", px, quality, 2, None),
                    Case(f"{n}_gray", np.ascontiguousarray(px[..., 1]), quality, 0, None)]
    return tuple(out)


@functools.lru_cache(None)
def crafted():
    """{name: Case} of every case but the pixel corpus"""
    cases = deep17() + deep18() + zero_runs() + dc_swing() + ac_max() + binary_noise() + long_eob()
    return {c.name: c for c in cases}


def channels(case):
    return 3 if case.px.ndim == 3 else 1
