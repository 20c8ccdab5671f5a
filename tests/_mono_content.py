"""Crafted Q16 gray inputs for the -monochrome kernels (fi_mono.hip), shared by
tests/test_mono_content_cpu.py (which proves on the oracle or the literal that
every input reaches the branch it was built for) and
tests/test_gpu_mono_content.py (which asks the kernels for the oracle's bytes
at every rotation).

Two devices make the content ownable:
  * owned stretch: an image that holds 0 and 65535, each more often than
    NormalizeImage's percentile thresholds, has (black, white) = (0, 65535),
    and the stretch of that pair is the identity -- so the image's histogram IS
    the stretched histogram the quantizer sees;
  * owned histogram: the pixels are laid out from a list of values, so the
    histogram is whatever the builder says; only the order (and so the dither)
    is left to a seeded shuffle.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as orc

ROTS = (0, 90, 180, 270)
SEAMS = (16384, 32768, 49152)  # fi_mono.hip builds the stretched histogram in four 16384-bin passes
EDGE_BINS = (1, 2, 127, 128, 129, 254, 255)
SEAM_BINS = (64, 127, 128, 191)


def q2c(q):
    """ScaleQuantumToChar of a Q16 value (works on arrays)."""
    q = np.asarray(q, dtype=np.int64)
    return ((q + 128) - ((q + 128) >> 8)) >> 8


def bin_lo():
    """lo[c] = the first Q16 value of 8-bit bin c, lo[256] = 65536."""
    c = q2c(np.arange(65536))
    return np.concatenate([np.searchsorted(c, np.arange(256)), [65536]]).astype(np.int64)


LO = bin_lo()


def hist_of(g):
    return np.bincount(np.asarray(g).ravel(), minlength=65536).astype(np.uint64)


def levels(g):
    """(black, white) of an image, by the oracle's or_mono_levels."""
    return orc.mono_levels(hist_of(g))


def stretched(g):
    """the oracle's stretched image (or_mono_levels + or_mono_stretch)."""
    g = np.asarray(g, dtype=np.uint16)
    b, w = levels(g)
    lut = np.array([orc.mono_stretch(int(q), b, w) for q in np.unique(g)], dtype=np.uint16)
    return lut[np.searchsorted(np.unique(g), g)]


def leaves(g):
    """number of 8-bit leaves (ClassifyImageColors' colors) of the stretched image."""
    return int(np.unique(q2c(stretched(g))).size)


def own(H):
    """Raise H[0] and H[65535] until (black, white) = (0, 65535) whatever else
    H holds: H[0] > n * 0.0015 and H[65535] > n - n * 0.9995."""
    H = np.array(H, dtype=np.int64)
    while True:
        n = float(H.sum())
        bp, wt = n * 0.0015, n - n * 0.9995
        if H[0] > bp and H[65535] > wt:
            return H
        if not H[0] > bp:
            H[0] = int(bp) + 1
        if not H[65535] > wt:
            H[65535] = int(wt) + 1


def fold(n, rng, wmax=141, dmax=512):
    """A (h, w) with w * h >= n and neither side above dmax: a (1, n) strip
    would do, but the curve has 4^level steps (level 15 at n = 20000)."""
    w = int(rng.integers(-(-n // dmax), min(n, wmax) + 1))
    return -(-n // w), w


def factor(n, wmax=40):
    """(h, w) with w * h == n, w the largest divisor of n up to wmax"""
    w = max(d for d in range(1, wmax + 1) if n % d == 0)
    return n // w, w


def image_of(H, shape, rng):
    """The image of exactly histogram H (sum == h * w), pixel order shuffled."""
    H = np.asarray(H, dtype=np.int64)
    v = np.repeat(np.arange(65536), H)
    assert v.size == shape[0] * shape[1], (v.size, shape)
    rng.shuffle(v)
    return v.reshape(shape).astype(np.uint16)


def owned_image(H, rng, shape=None):
    """Own the stretch of H, fold it to a shape (padding with zeros, which stay
    owned) and lay it out."""
    H = own(H)
    if shape is None:
        shape = fold(int(H.sum()), rng)
    n = shape[0] * shape[1]
    H[0] += n - int(H.sum())
    while not H[65535] > n - n * 0.9995:  # the padding raised the white threshold
        H[65535] += 1
        H[0] -= 1
    assert H[0] > n * 0.0015 and H.sum() == n
    return image_of(H, shape, rng)


def _put(g, rng, pairs):
    """set count pixels to value for every (value, count), at distinct seeded places"""
    flat = g.reshape(-1)
    idx = rng.permutation(flat.size)[: sum(c for _, c in pairs)]
    k = 0
    for v, c in pairs:
        flat[idx[k : k + c]] = v
        k += c
    return g


# ---- levels ------------------------------------------------------------------------
def levels_strict():
    """n = 2000: bp = 3.0 and n - wp = 1.0; n = 4000: 6.0 and 2.0 (exact in f64).
    name -> (image, (black, white)): a count equal to the threshold does not
    pass it (strict >), one pixel more does.  The flat fill of 30000 dithers to
    the same bytes whichever of 100 and 200 is black; the noise fill does not.
    k_mono_stats searches a coarse bin (q >> 8) and then its 256 values:
    100 / 200 and 60000 / 59990 share a coarse bin, 100 / 300 and 60000 / 50000
    do not, so the count meets the threshold inside a bin and at its end."""
    out = {}
    for n, shape, kb, kw in ((2000, (40, 50), 3, 1), (4000, (50, 80), 6, 2)):
        for name, db, dw in (("at", 0, 0), ("low_plus1", 1, 0), ("high_plus1", 0, 1)):
            for fill in ("", "_noise"):
                rng = np.random.default_rng(n + db + 2 * dw)
                g = rng.integers(1000, 49000, shape).astype(np.uint16) if fill else np.full(shape, 30000, np.uint16)
                _put(g, rng, [(100, kb + db), (200, 1), (60000, kw + dw), (50000, 1)])
                out[f"n{n}_{name}{fill}"] = (g, (100 if db else 200, 60000 if dw else 50000))
        for name, db, dw in (("at", 0, 0), ("low_plus1", 1, 0), ("high_plus1", 0, 1)):
            rng = np.random.default_rng(n + db + 2 * dw + 50)
            g = rng.integers(1000, 49000, shape).astype(np.uint16)
            _put(g, rng, [(100, kb + db), (300, 1), (60000, kw + dw), (59990, 1)])
            out[f"n{n}_{name}_other_bin_noise"] = (g, (100 if db else 300, 60000 if dw else 59990))
    return out


def levels_collapse():
    rng = np.random.default_rng(77)
    a = _put(np.zeros((50, 50), np.uint16), rng, [(300, 1)])
    b = _put(np.full((50, 50), 65535, np.uint16), rng, [(40000, 1)])
    c = _put(np.full((40, 50), 20000, np.uint16), rng, [(5, 1), (60000, 1)])
    d = np.where(rng.random((20, 20)) > 0.5, 10001, 10000).astype(np.uint16)
    return {"white_falls_to_0": a, "both_65535": b, "one_colour_20000": c, "adjacent_values": d}


def almost_bilevel():
    """name -> (image, the (y, x) of the one non-bilevel pixel or None)"""
    rng = np.random.default_rng(1234)
    noise = np.where(rng.random((31, 33)) > 0.5, 65535, 0).astype(np.uint16)
    yy, xx = np.mgrid[0:31, 0:33]
    checker = np.where((xx + yy) & 1, 65535, 0).astype(np.uint16)
    out = {}
    for nm, base in (("noise", noise), ("checker", checker)):
        out[f"{nm}_bilevel"] = (base, None)
        for v in (1, 7):
            at = (int(rng.integers(0, 31)), int(rng.integers(0, 33)))
            g = base.copy()
            g[at] = v
            out[f"{nm}_one_px_{v}"] = (g, at)
    return out


# ---- owned histograms --------------------------------------------------------------
def seam_hist(bins, rng):
    H = np.zeros(65536, np.int64)
    for c in bins:
        H[LO[c] : LO[c + 1]] = rng.integers(1, 6, LO[c + 1] - LO[c])
    for s in SEAMS:
        H[s - 1] += int(rng.integers(1, 6)) * (H[s - 1] == 0)
        H[s] += int(rng.integers(1, 6)) * (H[s] == 0)
    return H


def quarter_seams():
    """name -> image: the six values either side of a 16384-bin seam, and all of
    the 8-bit bins on one: 64 and 191 straddle theirs, 127 ends on 32768 and
    128 begins on it (LO[128] == 32768); counts 1..5"""
    out = {}
    for name, bins in (("all", SEAM_BINS), ("bin64", (64,)), ("bin127_128", (127, 128)), ("bin191", (191,)),
                       ("six", ())):
        rng = np.random.default_rng(600 + len(name) + sum(bins))
        out[name] = owned_image(seam_hist(bins, rng), rng)
        H = seam_hist(bins, rng)
        np.add.at(H, rng.integers(0, 65536, 400), 1)  # the same beside a full tree
        out[name + "_in_noise"] = owned_image(H, rng)
    return out


def bin_edges():
    """lo[c] - 1 and lo[c] for the bins of EDGE_BINS: neighbours in Q16, different 8-bit leaves"""
    out = {}
    for seed in (1, 2):
        rng = np.random.default_rng(700 + seed)
        H = np.zeros(65536, np.int64)
        for c in EDGE_BINS:
            H[LO[c] - 1] = int(rng.integers(1, 6))
            H[LO[c]] = int(rng.integers(1, 6))
        for q in (127, 128, 384, 385, 65407, 65408):  # 257 c - 129 and its neighbour, off the edge by one
            H[q] = max(H[q], 1)
        out[f"edges_{seed}"] = owned_image(H, rng, shape=None if seed == 1 else (1, int(own(H).sum())))
    return out


def symmetric_hists():
    """name -> histogram with H[q] == H[65535 - q]"""
    out = {}
    for seed in range(6):
        rng = np.random.default_rng(800 + seed)
        H = np.zeros(65536, np.int64)
        np.add.at(H, rng.integers(1, 32768, 287), 1)  # 287 + the 0: half of 24 x 24
        H[0] = 1
        out[f"random_half_{seed}"] = H + H[::-1]  # 576 pixels: one 0 and one 65535 own the stretch
    for seed, step in ((0, 1), (1, 5), (2, 17), (3, 51), (4, 85)):
        rng = np.random.default_rng(850 + seed)
        H = np.zeros(65536, np.int64)
        k = np.arange(0, 128, step)
        H[257 * k] = rng.integers(1, 4, k.size)
        H[0] = 3  # owns the stretch up to 1999 pixels
        out[f"mult257_step{step}"] = H + H[::-1]
    return out


def symmetric_ties():
    out = {}
    for name, H in symmetric_hists().items():
        n = int(H.sum())
        out[name] = image_of(H, (24, 24) if n == 576 else factor(n), np.random.default_rng(n + len(name)))
    return out


def few_colours():
    """name -> (image, distinct values, 8-bit leaves of the stretched image).
    A dominant value with at most 3 pixels below and 1 above (n = 2500:
    bp = 3.75, n - wp = 1.25) has black == white: nothing is stretched and the
    values keep their leaves; anything else is stretched to 0 .. 65535."""
    rng = np.random.default_rng(31)
    out = {}

    def dom(v, others):
        return _put(np.full((50, 50), v, np.uint16), rng, [(o, 1) for o in others])

    out["v2_leaf1"] = (dom(30000, [30001]), 2, 1)
    out["v3_leaf1"] = (dom(30000, [29999, 30001]), 3, 1)
    out["v4_leaf1"] = (dom(30000, [29998, 29999, 30001]), 4, 1)
    e = int(LO[118])  # 30198: the first value of bin 118
    out["v2_leaf2"] = (dom(e - 1, [e]), 2, 2)
    out["v3_leaf2"] = (dom(e, [e - 2, e - 1]), 3, 2)
    out["v4_leaf2"] = (dom(e, [e - 2, e - 1, e + 1]), 4, 2)
    out["v2_stretched_leaf2"] = (np.where(rng.random((20, 20)) > 0.3, 50000, 10000).astype(np.uint16), 2, 2)
    for name, vals, lv in (("v3_owned_leaf2", (0, 40, 65535), 2), ("v4_owned_leaf2", (0, 40, 65500, 65535), 2),
                           ("v3_owned_leaf3", (0, 20000, 65535), 3), ("v4_owned_leaf3", (0, 20000, 20100, 65535), 3),
                           ("v4_owned_leaf4", (0, 20000, 40000, 65535), 4)):
        H = np.zeros(65536, np.int64)
        H[list(vals)] = rng.integers(20, 200, len(vals))
        out[name] = (owned_image(H, rng), len(vals), lv)
    return out


def colour_order():
    yy, xx = np.mgrid[0:33, 0:47]
    ramp = (xx * 65535 // 46 + yy % 3).clip(0, 65535).astype(np.uint16)
    rng = np.random.default_rng(41)
    skew = np.minimum(65535, (rng.random((33, 47)) ** 3 * 70000).astype(np.int64)).astype(np.uint16)
    return {"ramp": ramp, "skewed": skew}


def cache_and_clamps():
    rng = np.random.default_rng(51)
    return {
        "noise": rng.integers(0, 65536, (47, 33)).astype(np.uint16),
        "narrow": rng.integers(21000, 26000, (47, 33)).astype(np.uint16),
        "three_values": rng.choice(np.array([1000, 30000, 64000], np.uint16), (47, 33)),
    }


SWEEP = 200
SWEEP_KINDS = ("random", "mirrored", "mult257", "bilevel_plus", "cluster", "few", "mirrored_mult257")


def sweep_hist(seed):
    """one of the 200 histograms of histogram_sweep (not yet owned)"""
    rng = np.random.default_rng(9000 + seed)
    kind = SWEEP_KINDS[seed % len(SWEEP_KINDS)]
    H = np.zeros(65536, np.int64)
    cmax = int(rng.choice([1, 3, 20, 1000]))
    if kind == "random":
        q = rng.integers(0, 65536, int(rng.integers(2, 400)))
    elif kind == "mirrored":
        q = rng.integers(0, 32768, int(rng.integers(1, 200)))
    elif kind == "mult257":
        q = 257 * rng.integers(0, 256, int(rng.integers(2, 120)))
    elif kind == "mirrored_mult257":  # few terms per node: the mirrored sums round alike and tie
        q = 257 * rng.integers(0, 128, int(rng.integers(1, 13)))
    elif kind == "bilevel_plus":
        q = rng.integers(1, 65535, int(rng.integers(1, 5)))
        cmax = min(cmax, 3)
    elif kind == "cluster":
        q = int(rng.integers(0, 65036)) + rng.integers(0, 500, int(rng.integers(2, 300)))
    else:
        q = rng.integers(0, 65536, int(rng.integers(1, 41)))
    q = np.unique(q)
    cnt = rng.integers(1, cmax + 1, q.size)
    cnt = np.maximum(1, cnt * min(1.0, 9000.0 / cnt.sum())).astype(np.int64)  # n capped (mirror doubles it)
    H[q] = cnt
    if kind.startswith("mirrored"):
        H = H + H[::-1]
    if kind == "bilevel_plus":
        H[0] += int(rng.integers(50, 2000))
        H[65535] += int(rng.integers(50, 2000))
    return kind, H


def sweep_image(seed):
    """(kind, image, its histogram): owned stretch, so the histogram is also the stretched one"""
    kind, H = sweep_hist(seed)
    rng = np.random.default_rng(19000 + seed)
    if kind.startswith("mirrored"):  # own and pad in pairs: the histogram stays its own mirror
        H = own(H)
        H[0] = H[65535] = max(H[0], H[65535])
        h, w = fold(int(H.sum()) // 2, rng, 70, 256)
        pad = h * w - int(H.sum()) // 2
        H[0] += pad
        H[65535] += pad
        g = image_of(H, (h, 2 * w), rng)
    else:
        g = owned_image(H, rng)
    assert g.size <= 20000 and max(g.shape) <= 1025
    return kind, g, hist_of(g)


CURVE_SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (4, 4), (5, 4), (8, 8), (9, 7), (17, 1), (1, 17), (31, 33),
                (32, 32), (33, 32), (63, 65), (64, 64), (65, 3), (128, 2), (129, 5), (256, 1), (257, 2), (2, 511),
                (512, 2), (1, 513), (1025, 2)]  # (w, h)


def curve_geometry():
    """'WxH' -> noise; from 4 pixels on with the stretch owned (1 x 1 is one
    value, the two-pixel strips would be bilevel if they held 0 and 65535)"""
    out = {}
    for w, h in CURVE_SHAPES:
        rng = np.random.default_rng(100 * w + h)
        g = rng.integers(1, 65535, (h, w)).astype(np.uint16)
        n = w * h
        if n >= 4:
            _put(g, rng, [(0, int(n * 0.0015) + 1), (65535, int(n - n * 0.9995) + 1)])
        out[f"{w}x{h}"] = g
    return out


def kernel_cases():
    """every part-A input but the sweep: 'group/name' -> image"""
    out = {}

    def add(group, d):
        for k, v in d.items():
            out[f"{group}/{k}"] = v[0] if isinstance(v, tuple) else v

    add("levels_strict", levels_strict())
    add("levels_collapse", levels_collapse())
    add("almost_bilevel", almost_bilevel())
    add("quarter_seams", quarter_seams())
    add("bin_edges", bin_edges())
    add("symmetric_ties", symmetric_ties())
    add("few_colours", few_colours())
    add("colour_order", colour_order())
    add("cache_and_clamps", cache_and_clamps())
    add("curve_geometry", curve_geometry())
    return out


# a 3-row strip, a full dither and the bilevel pass-through (noise: the checker is its own 90 <-> 270 swap)
WIDE_STRIDE = ("curve_geometry/65x3", "cache_and_clamps/noise", "almost_bilevel/noise_bilevel")


# ---- pipeline batch ----------------------------------------------------------------
def pipeline_batch():
    """Part B: (name, RGB source, target_w, target_h, fill + extent, rotate,
    monochrome).  Identity geometry throughout (the target is the source size,
    or a fill + extent window of it), so the Q16 gray that reaches the stage is
    exact on both sides."""
    rng = np.random.default_rng(61)

    def gray3(v):
        return np.repeat(np.asarray(v, np.uint8)[..., None], 3, axis=2)

    return [
        ("one_px_rot0", gray3(rng.integers(1, 255, (1, 1))), 1, 1, False, 0, True),
        ("gray_noise_17x33_rot90", gray3(rng.integers(0, 256, (33, 17))), 17, 33, False, 90, True),
        ("colour_noise_100x50_rot180", rng.integers(0, 256, (50, 100, 3)).astype(np.uint8), 100, 50, False, 180, True),
        ("bilevel_64x64_rot270", gray3(np.where(rng.random((64, 64)) > 0.5, 255, 0)), 64, 64, False, 270, True),
        ("plain_rgb_40x30", rng.integers(0, 256, (30, 40, 3)).astype(np.uint8), 40, 30, False, 0, False),
        ("strip_257x3_rot90", gray3(rng.integers(0, 256, (3, 257))), 257, 3, False, 90, True),
        ("window_60x50_rot180", rng.integers(0, 256, (50, 100, 3)).astype(np.uint8), 60, 50, True, 180, True),
        ("uniform_128_17x33_rot270", gray3(np.full((33, 17), 128)), 17, 33, False, 270, True),
        ("colour_noise_64x64_rot0", rng.integers(0, 256, (64, 64, 3)).astype(np.uint8), 64, 64, False, 0, True),
    ]


def pipeline_reference(src, tw, th, window, rot, mono):
    """the oracle's convert of one pipeline_batch entry"""
    f = orc.FLAG_THUMBNAIL | (orc.FLAG_MONO if mono else 0) | (orc.FLAG_ROTATE if rot else 0)
    if window:
        f |= orc.FLAG_FILL | orc.FLAG_EXTENT
    return orc.im_convert(src, tw, th, f, rotate=rot)
