"""The smart-crop score kernels (fi_sc_score.hip: k_sc_score3, k_sc_score2<1>,
k_sc_score2<0>) against the oracle on the crafted content of
tests/_score_content.py, whose claims tests/test_score_content_cpu.py proves
on the oracle alone: sources whose crops tie (so the candidate list, the exact
re-score and the first-maximum rule decide the box), geometries on every
branch of plan_score_groups, non-default parameters, and a mixed batch.

Every case runs with ``prescale = 0`` on two contexts -- the default one, whose
score kernel the case table states and the context's counters confirm (no
silent fallback), and FI_SC_MFMA=0 (k_sc_score2 forced) -- and with
``exact_all`` 0 and 1.  Asserted each time:
  * the crop list and the top index are the oracle's;
  * a crop with exact == 1 carries the oracle's detail, saturation, skin and
    total bit for bit; one with exact == 0 lies within 1e-9 * max(1, |total|)
    of it (the fast-pass tolerance test_gpu_parity.py states);
  * the bound is sound: where at least two crops share the maximum bit for bit,
    every one of them was re-scored (two crops with the same exact total have
    overlapping intervals, so both must have been candidates);
  * both contexts agree field for field where the result is exact, and within
    the tolerance where it is a fast total.
Each case prints the kernel it reached and the number of candidates seen
(``pytest -s``); those figures are recorded, not asserted.
"""
import numpy as np
import pytest

from flyimg_amd import _lib as L
from flyimg_amd.runtime import Op
from tests import _score_content as C
from tests.test_gpu_parity import _ENV, SC_PATHS, _context_with, _opts

pytestmark = pytest.mark.gpu

W, H = C.TIE_W, C.TIE_H
FIELDS = ("detail", "saturation", "skin", "total")


@pytest.fixture(scope="module")
def dctx():
    """the default kernels (k_sc_score3 where the planner finds groups)"""
    c = _context_with(SC_PATHS["vr"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def vctx():
    """k_sc_score2 forced"""
    c = _context_with(dict(_ENV, FI_SC_MFMA="0"))
    yield c
    c.close()


def _options(options, exact_all):
    o = _opts(exact_all)
    o.prescale = 0
    for k, v in options.items():
        setattr(o, k, v)
    return o


def _params(overrides):
    if not overrides:
        return None
    p = L.FiSmartcropParams()
    L.lib().fi_smartcrop_default_params(p)
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


def _close(a, b):
    return abs(a - b) <= 1e-9 * max(1.0, abs(b))


def _check(r, ref, exact_all):
    crops = ref["crops"]
    assert r["n"] == len(crops)
    assert list(r["analyse_size"]) == list(ref["analyse_size"]) and r["prescale"] == 1.0
    for c, g in zip(r["crops"], crops):
        assert [c.x, c.y, c.width, c.height] == [g["x"], g["y"], g["width"], g["height"]]
    assert r["top_index"] == ref["top_index"]
    for k, (c, g) in enumerate(zip(r["crops"], crops)):
        assert c.exact in (0, 1), (k, c.exact)
        if c.exact:
            assert [getattr(c, f).hex() for f in FIELDS] == [g["score"][f].hex() for f in FIELDS], k
        else:
            assert _close(c.total, g["score"]["total"]), (k, c.total, g["score"]["total"])
    tied = C.exact_ties(ref)
    if len(tied) >= 2:
        assert [k for k in tied if not r["crops"][k].exact] == []
        assert r["crops"][r["top_index"]].exact == 1
    if exact_all:
        assert all(c.exact == 1 for c in r["crops"])


def _agree(a, b, ref):
    """two contexts' results field for field; fast totals within the tolerance
    (a single candidate keeps its fast total, the top crop's included: the
    two fast passes differ there, and _check holds each to the oracle)"""
    assert a["n"] == b["n"] and a["top_index"] == b["top_index"]
    tied = set(C.exact_ties(ref)) if len(C.exact_ties(ref)) >= 2 else set()
    ta, tb = a["crops"][a["top_index"]], b["crops"][b["top_index"]]
    if ta.exact and tb.exact:
        assert ta.total.hex() == tb.total.hex()
    for k, (x, y) in enumerate(zip(a["crops"], b["crops"])):
        assert [x.x, x.y, x.width, x.height] == [y.x, y.y, y.width, y.height]
        if k in tied:
            assert x.exact == y.exact == 1
        if x.exact and y.exact:
            assert [getattr(x, f).hex() for f in FIELDS] == [getattr(y, f).hex() for f in FIELDS], k
        else:
            assert _close(x.total, y.total), (k, x.total, y.total)


def _counted(ctx, want, fn):
    """fn() ran one image on the score kernel counted by `want`, none on the other"""
    before = {k: ctx.stats(k)[1] for k in (C.MFMA, C.VALU)}
    r = fn()
    ran = {k: ctx.stats(k)[1] - before[k] for k in before}
    assert ran == {want: 1, (C.VALU if want == C.MFMA else C.MFMA): 0}, (want, ran)
    return r


def _run(dctx, vctx, name, img, ref, kernel, tw=100, th=100, options=None, params=None, all_exact=False):
    options = options or {}
    want = C.MFMA if kernel == C.S3 else C.VALU
    seen = {}
    for exact_all in (0, 1):
        o, p = _options(options, exact_all), _params(params)
        rd = _counted(dctx, want, lambda: dctx.smartcrop_ex(img, tw, th, params=p, options=o))
        rv = _counted(vctx, C.VALU, lambda: vctx.smartcrop_ex(img, tw, th, params=p, options=o))
        for r in (rd, rv):
            _check(r, ref, exact_all or all_exact)
        _agree(rd, rv, ref)
        if not exact_all:
            seen = {k: max(1, sum(c.exact for c in r["crops"])) for k, r in (("default", rd), ("valu", rv))}
    print(f"\nscore-content {name}: {kernel} crops {len(ref['crops'])} exact ties {len(C.exact_ties(ref))} "
          f"n_candidates {seen['default']} (k_sc_score2 forced: {seen['valu']})")


# ---- 1. content that ties -------------------------------------------------------
@pytest.mark.parametrize("case", C.TIE_CASES, ids=[c.name for c in C.TIE_CASES])
def test_tie_content(dctx, vctx, case):
    ref = C.ref_for(case.source, W, H, params=case.params)
    _run(dctx, vctx, case.name, C.SOURCES[case.source](W, H), ref, case.kernel, params=case.params)


# ---- 2./3. geometries on every planner branch ------------------------------------
GEO = [(g, content) for g in C.GEO_CASES for content in C.GEO_CONTENT] + \
      [(g, content) for name, content in C.GEO_EXTRA for g in C.GEO_CASES if g.name == name]


@pytest.mark.parametrize("case,content", GEO, ids=[f"{g.name}-{content}" for g, content in GEO])
def test_geometry(dctx, vctx, case, content):
    ref = C.ref_for(content, case.W, case.H, case.tw, case.th, case.options)
    _run(dctx, vctx, f"{case.name}-{content}", C.SOURCES[content](case.W, case.H), ref, case.kernel,
         case.tw, case.th, case.options)


# ---- 4. parameters -----------------------------------------------------------------
PARAMS = [(p, content) for p in C.PARAM_CASES for content in C.PARAM_CONTENT]


@pytest.mark.parametrize("case,content", PARAMS, ids=[f"{p.name}-{content}" for p, content in PARAMS])
def test_params(dctx, vctx, case, content):
    """non-default fi_smartcrop_params reach ScParamsDev, the importance tables,
    the B fragments and the bound; with a negative bias (fast_ok false) every
    crop comes back re-scored"""
    ref = C.ref_for(content, W, H, params=case.params)
    _run(dctx, vctx, f"{case.name}-{content}", C.SOURCES[content](W, H), ref, case.kernel, params=case.params,
         all_exact=case.all_exact)


@pytest.mark.parametrize("w,h,k,kernel", C.TUNED_CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}" for c in C.TUNED_CASES])
def test_tuned_weight_near_tie_of_unrelated_crops(dctx, vctx, w, h, k, kernel):
    """two crops of a noise image a few ulps apart (a detail_weight bisected to
    the crossing of their totals; the top crop differs between the two adjacent
    weights): their fast totals err independently, so a bound below the fast
    pass's real error, or a re-score that is not the oracle's sum, picks the
    wrong box on one side or the other"""
    img = C.noise(w, h)
    for side, wd in zip("ab", C.weight_crossings(w, h)[k]):
        p = {"detail_weight": wd}
        _run(dctx, vctx, f"tuned-{w}x{h}-{k}{side}", img, C.ref_for("noise", w, h, params=p), kernel, params=p)


# ---- 5. a batch ----------------------------------------------------------------------
@pytest.mark.parametrize("which", ["default", "valu"])
def test_batch_records_do_not_depend_on_position(dctx, vctx, which):
    """Context.process with the smartcrop flag, no resize and no apply: tie
    sources, controls and four plans in one batch, forwards and reversed.  The
    prescale is the identity for these targets (CPU file), so the scored
    pixels are the source's."""
    from oracle import oracle as orc

    ctx = dctx if which == "default" else vctx
    imgs = [C.SOURCES[s](w, h) for s, w, h, _ in C.BATCH]
    ops = [Op(0, 0, L.FI_OP_SMARTCROP, L.GRAVITY["Center"], 0, t, t) for _, _, _, t in C.BATCH]
    refs = [orc.sc_crop(img, t, t) for img, (_, _, _, t) in zip(imgs, C.BATCH)]
    want = [C.planned(ref, w, h, 8).counter if which == "default" else C.VALU
            for ref, (_, w, h, _) in zip(refs, C.BATCH)]
    got = {}
    for order in (list(range(len(imgs))), list(reversed(range(len(imgs))))):
        before = {k: ctx.stats(k)[1] for k in (C.MFMA, C.VALU)}
        outs, recs, rc = ctx.process([imgs[i] for i in order], [ops[i] for i in order])
        assert rc == 0, L.lib().fi_last_error()
        ran = {k: ctx.stats(k)[1] - before[k] for k in before}
        assert ran == {k: want.count(k) for k in before}, ran
        for pos, i in enumerate(order):
            rec, ref, (source, w, h, t) = recs[pos], refs[i], C.BATCH[i]
            assert rec.status == 0 and np.array_equal(outs[pos], imgs[i])
            top = ref["top_crop"]
            assert (rec.crop_x, rec.crop_y, rec.crop_w, rec.crop_h) == \
                (top["x"], top["y"], top["width"], top["height"]), (source, w, h)
            if rec.n_candidates > 1:
                assert rec.crop_score.hex() == top["score"]["total"].hex(), (source, w, h)
            else:
                assert rec.n_candidates == 1 and _close(rec.crop_score, top["score"]["total"])
            if source not in C.BATCH_UNTIED:
                assert rec.n_candidates >= 2, (source, w, h)
            key = (rec.crop_x, rec.crop_y, rec.crop_w, rec.crop_h, rec.crop_score.hex(), rec.n_candidates)
            assert got.setdefault(i, key) == key, (source, w, h, pos)
    print(f"\nscore-content batch ({which}): n_candidates " +
          " ".join(f"{s}@{w}x{h}/{t}={got[i][5]}" for i, (s, w, h, t) in enumerate(C.BATCH)))
