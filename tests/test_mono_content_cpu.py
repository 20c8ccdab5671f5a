"""CPU proofs for tests/_mono_content.py: every crafted -monochrome input
reaches the branch it was built for, shown on the oracle (oracle/fi_oracle.c)
or on the literal restatement (tests/mono_literal.py, whose info dict reports
what a run met) before tests/test_gpu_mono_content.py relies on it.  The
figures printed here for the committed seeds are the ones in DESIGN.md § 4."""
import math

import numpy as np
import pytest

from oracle import oracle as orc
from tests import _mono_content as C
from tests import mono_literal as ml


def _literal(g):
    info = {}
    out = ml.monochrome(g, exact_sums=True, info=info)
    return out, info


def test_info_leaves_the_literal_as_it_was():
    g = C.cache_and_clamps()["narrow"][:12, :9]
    out, info = _literal(g)
    assert np.array_equal(out, ml.monochrome(g, exact_sums=True))
    assert set(info) == {"bilevel", "black", "white", "cmap", "clamp_lo", "clamp_hi", "stale", "excluded"}
    info = {}
    ml.monochrome(np.array([[0, 65535]], np.uint16), info=info)
    assert info == {"bilevel": True}


def test_owned_stretch_is_the_identity():
    assert all(orc.mono_stretch(q, 0, 65535) == q for q in range(65536))


def test_bin_bounds():
    """LO is the q range of each 8-bit bin, the table k_mono_stats builds by increment"""
    c = C.q2c(np.arange(65536))
    assert C.LO[0] == 0 and C.LO[256] == 65536 and np.all(np.diff(C.LO) > 0)
    for b in range(256):
        assert c[C.LO[b]] == b and c[C.LO[b + 1] - 1] == b
    assert [int(C.LO[b]) for b in (1, 2, 128, 255)] == [129, 386, 32768, 65407]


# ---- levels ------------------------------------------------------------------------
def test_levels_strict():
    cases = C.levels_strict()
    assert 2000 * 0.0015 == 3.0 and 2000 - 2000 * 0.9995 == 1.0
    assert 4000 * 0.0015 == 6.0 and 4000 - 4000 * 0.9995 == 2.0
    for name, (g, want) in cases.items():
        assert C.levels(g) == want, name
        info = {}
        ml.stretch(g, info)
        assert (info["black"], info["white"]) == want, name
    for n in (2000, 4000):
        at, lo, hi = (cases[f"n{n}_{k}"][1] for k in ("at", "low_plus1", "high_plus1"))
        assert at == (200, 50000) and lo == (100, 50000) and hi == (200, 60000)


def test_levels_strict_shows_in_the_bytes(monkeypatch):
    """A search that stops at a count equal to its threshold (>= for >) gives
    other bytes: shown on the literal with the stretch of the wrong pair put in
    its place.  The flat fill hides the black point (100 or 200, the same
    bytes), which is why the noise fills are there."""
    cases = C.levels_strict()
    seen = {"black": 0, "white": 0, "flat_black_hidden": 0}
    for name, (g, (black, white)) in cases.items():
        H = C.hist_of(g).astype(np.float64)
        n = float(g.size)
        wrong_black = int(np.argmax(np.cumsum(H) >= n * 0.0015))
        wrong_white = 65535 - int(np.argmax(np.cumsum(H[::-1]) >= n - n * 0.9995))
        good = ml.monochrome(g, exact_sums=True)
        for which, pair in (("black", (wrong_black, white)), ("white", (black, wrong_white))):
            if pair == (black, white):
                assert "plus1" in name  # one pixel more: both forms agree
                continue
            lut = np.array([orc.mono_stretch(q, *pair) for q in range(65536)], np.uint16)
            monkeypatch.setattr(ml, "stretch", lambda img, info=None, lut=lut: lut[img])
            differs = not np.array_equal(ml.monochrome(g, exact_sums=True), good)
            monkeypatch.undo()
            if which == "black" and "noise" not in name:
                assert not differs
                seen["flat_black_hidden"] += 1
            else:
                assert differs, (name, which)
                seen[which] += 1
    assert seen == {"black": 8, "white": 12, "flat_black_hidden": 4}, seen


def test_levels_collapse():
    c = C.levels_collapse()
    out, info = _literal(c["white_falls_to_0"])
    assert C.levels(c["white_falls_to_0"]) == (0, 0) == (info["black"], info["white"])
    assert not info["bilevel"] and not out.any()
    out, info = _literal(c["both_65535"])
    assert C.levels(c["both_65535"]) == (65535, 65535) == (info["black"], info["white"])
    assert not info["bilevel"] and np.all(out == 255)
    out, info = _literal(c["one_colour_20000"])
    assert C.levels(c["one_colour_20000"]) == (20000, 20000)
    assert len(info["cmap"]) == 1 and not out.any() and info["clamp_lo"] > 1900
    assert orc.mono_quant_info(C.hist_of(c["one_colour_20000"]))[0] == 1
    out, info = _literal(c["adjacent_values"])
    assert C.levels(c["adjacent_values"]) == (10000, 10001) and sorted(info["cmap"]) == [0, 65535]
    assert set(np.unique(C.stretched(c["adjacent_values"]))) == {0, 65535}
    for name, g in c.items():
        assert np.array_equal(orc.im_monochrome(g), ml.monochrome(g, exact_sums=True)), name
        print(name, C.levels(g), _literal(g)[1])


def test_almost_bilevel():
    for name, (g, at) in C.almost_bilevel().items():
        out, info = _literal(g)
        ref = orc.im_monochrome(g)
        assert np.array_equal(out, ref), name
        if at is None:
            assert info == {"bilevel": True} and np.array_equal(ref, np.where(g > 0, 255, 0))
            continue
        nb = (g != 0) & (g != 65535)
        assert nb.sum() == 1 and nb[at] and not info["bilevel"]
        assert (info["black"], info["white"]) == (0, 65535)
        assert ref[at] == 0, name


# ---- owned histograms --------------------------------------------------------------
def test_quarter_seams():
    assert C.LO[64] < 16384 < C.LO[65] and C.LO[191] < 49152 < C.LO[192]
    assert C.LO[128] == 32768  # this seam is a bin edge: 127 ends on it, 128 begins on it
    for name, g in C.quarter_seams().items():
        H = C.hist_of(g)
        assert C.levels(g) == (0, 65535), name
        for s in C.SEAMS:
            assert H[s - 1] and H[s], name
        for c in C.SEAM_BINS:
            if f"{c}" in name or name.startswith("all"):
                assert np.all(H[C.LO[c] : C.LO[c + 1]] >= 1), name
        if not name.endswith("_in_noise"):
            assert H[1:65535].max() <= 5
        n, means, _ = orc.mono_quant_info(H)
        out, info = _literal(g)
        assert info["cmap"] == means and np.array_equal(out, orc.im_monochrome(g)), name
        print(name, g.shape, "ncol", n, means)


def test_bin_edges():
    for c in C.EDGE_BINS:
        assert C.q2c(C.LO[c] - 1) == c - 1 and C.q2c(C.LO[c]) == c
    assert [int(C.LO[c]) for c in C.EDGE_BINS] == [129, 386, 32511, 32768, 33025, 65150, 65407]
    for name, g in C.bin_edges().items():
        H = C.hist_of(g)
        assert C.levels(g) == (0, 65535), name
        assert all(H[C.LO[c] - 1] and H[C.LO[c]] for c in C.EDGE_BINS), name
        assert np.array_equal(orc.im_monochrome(g), ml.monochrome(g, exact_sums=True)), name


def _mid(L, c):
    mid, bisect = 65535.0 / 2.0, (65535.0 + 1.0) / 2.0
    for lv in range(1, L + 1):
        bisect *= 0.5
        mid += bisect if (c >> (8 - lv)) & 1 else -bisect
    return mid


def _node_errors(H):
    """(level, prefix) -> quantize error, in the oracle's order: per (level, bin)
    partials over ascending q, then per node over ascending bins"""
    err = {}
    qs = np.nonzero(H)[0]
    cs = C.q2c(qs)
    for L in range(1, 9):
        for c in np.unique(cs):
            mid, part = _mid(L, int(c)), 0.0
            for q in qs[cs == c]:
                e = (1.0 / 65535.0) * (float(q) - mid)
                d = e * e + e * e
                d = d + e * e
                part += float(H[q]) * math.sqrt(d)
            key = (L, int(c) >> (8 - L))
            err[key] = err.get(key, 0.0) + part
    return err


def test_symmetric_ties():
    ncols = set()
    imgs = C.symmetric_ties()
    for name, H in C.symmetric_hists().items():
        g = imgs[name]
        assert np.array_equal(H, H[::-1]) and np.array_equal(C.hist_of(g), H.astype(np.uint64)), name
        assert C.levels(g) == (0, 65535), name
        err = _node_errors(H)
        pairs = [(k, (k[0], (1 << k[0]) - 1 - k[1])) for k in err if k[1] < (1 << k[0]) - 1 - k[1]]
        tied = sum(err[a] == err[b] for a, b in pairs)
        assert tied > 0 and all(b in err for _, b in pairs), name
        n = orc.mono_quant_info(H)[0]
        ncols.add(n)
        print(name, g.shape, "mirror pairs", len(pairs), "bit-equal", tied, "ncol", n)
    assert ncols == {1, 2}
    assert imgs["random_half_0"].shape[0] * imgs["random_half_0"].shape[1] == 24 * 24


def test_few_colours():
    for name, (g, values, lv) in C.few_colours().items():
        assert np.unique(g).size == values and C.leaves(g) == lv, name
        assert np.array_equal(orc.im_monochrome(g), ml.monochrome(g, exact_sums=True)), name
    got = {(v, lv) for _, v, lv in C.few_colours().values()}
    assert {(2, 1), (3, 1), (4, 1), (2, 2), (3, 2), (4, 2), (3, 3), (4, 3), (4, 4)} <= got


def test_colour_order():
    c = C.colour_order()
    for name, dark_first in (("ramp", False), ("skewed", True)):
        out, info = _literal(c[name])
        m = info["cmap"]
        assert len(m) == 2 and (m[0] < m[1]) == dark_first, (name, m)
        assert orc.mono_quant_info(C.hist_of(C.stretched(c[name])))[1] == m
        assert np.array_equal(out, orc.im_monochrome(c[name]))
        print(name, m)


def test_cache_and_clamps():
    for name, g in C.cache_and_clamps().items():
        out, info = _literal(g)
        assert np.array_equal(out, orc.im_monochrome(g)), name
        assert info["stale"] > 0 and info["clamp_lo"] > 0 and info["clamp_hi"] > 0, (name, info)
        print(name, info)  # "excluded" is recorded, not required


def test_histogram_sweep():
    ncol = {1: 0, 2: 0}
    kinds = {}
    for seed in range(C.SWEEP):
        kind, g, H = C.sweep_image(seed)
        assert g.size <= 20000 and max(g.shape) <= 1025, seed
        assert orc.mono_levels(H) == (0, 65535), seed
        if kind.startswith("mirrored"):
            assert np.array_equal(H, H[::-1]), seed
        n = orc.mono_quant_info(H)[0]
        ncol[n] += 1
        kinds[kind] = kinds.get(kind, 0) + 1
    print(ncol, kinds)
    assert min(ncol.values()) >= 20 and set(kinds) == set(C.SWEEP_KINDS)
    assert sorted(kinds) == sorted(set(C.sweep_hist(s)[0] for s in range(len(C.SWEEP_KINDS))))


def test_curve_geometry():
    imgs = C.curve_geometry()
    lv = {}
    for w, h in C.CURVE_SHAPES:
        g = imgs[f"{w}x{h}"]
        assert g.shape == (h, w) and g.size <= 4200
        lv.setdefault(orc.mono_curve_level(w, h), []).append(f"{w}x{h}")
        if g.size >= 4:
            assert C.levels(g) == (0, 65535), (w, h)
        assert np.array_equal(orc.im_monochrome(g), ml.monochrome(g, exact_sums=True)), (w, h)
    print(lv)
    assert sorted(lv) == list(range(1, 12))
    assert any(w == 1 for w, _ in C.CURVE_SHAPES) and any(h == 1 for _, h in C.CURVE_SHAPES)  # strips 1 px wide


def test_kernel_cases_are_complete():
    k = C.kernel_cases()
    groups = {n.split("/")[0] for n in k}
    assert groups == {"levels_strict", "levels_collapse", "almost_bilevel", "quarter_seams", "bin_edges",
                      "symmetric_ties", "few_colours", "colour_order", "cache_and_clamps", "curve_geometry"}
    assert all(n in k for n in C.WIDE_STRIDE) and len(C.WIDE_STRIDE) == 3
    assert all(v.dtype == np.uint16 and v.ndim == 2 and max(v.shape) <= 1025 for v in k.values())


# ---- part B: what makes the pipeline batch exact ---------------------------------------
def test_pipeline_batch_references():
    """Gray sources (R = G = B = v): the pipeline's reference is -monochrome of
    257 * v, rotations compose as np.rot90, and fill + extent crops the window
    first.  The batch holds what the issue lists."""
    batch = C.pipeline_batch()
    mono = [b for b in batch if b[6]]
    assert len(batch) >= 9 and len(mono) >= 8 and not batch[len(batch) // 2][6]
    for rot in C.ROTS:
        assert sum(b[5] == rot for b in mono) >= 2
    sizes = {(b[1].shape[1], b[1].shape[0], b[2], b[3]) for b in mono}
    assert {(1, 1, 1, 1), (17, 33, 17, 33), (100, 50, 100, 50), (64, 64, 64, 64), (257, 3, 257, 3),
            (100, 50, 60, 50)} <= sizes
    kinds = set()
    for name, src, tw, th, window, rot, is_mono in mono:
        ref = C.pipeline_reference(src, tw, th, window, rot, True)
        gray = np.all(src[..., 0] == src[..., 1]) and np.all(src[..., 0] == src[..., 2])
        v = src[..., 0]
        kinds.add("colour" if not gray else "bilevel" if np.all((v == 0) | (v == 255)) else
                  "uniform128" if np.all(v == 128) else "gray")
        if gray:
            q = v.astype(np.uint16) * 257
            if window:
                x0 = (src.shape[1] - tw) // 2
                q = q[:, x0 : x0 + tw]
                assert (x0, tw) == (20, 60)
            assert np.array_equal(ref, np.rot90(orc.im_monochrome(q), -rot // 90)), name
        else:
            assert np.array_equal(ref, np.rot90(C.pipeline_reference(src, tw, th, window, 0, True), -rot // 90)), name
    assert kinds == {"colour", "bilevel", "uniform128", "gray"}
    # the window case on a gray source too (the batch's one is colour noise)
    rng = np.random.default_rng(5)
    v = rng.integers(0, 256, (50, 100)).astype(np.uint8)
    src = np.repeat(v[..., None], 3, axis=2)
    assert np.array_equal(C.pipeline_reference(src, 60, 50, True, 0, True),
                          orc.im_monochrome(v[:, 20:80].astype(np.uint16) * 257))
