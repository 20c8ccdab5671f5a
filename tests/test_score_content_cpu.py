"""The crafted smart-crop score content (tests/_score_content.py) does what
its names claim -- proved on the CPU oracle alone, so the GPU file
(tests/test_gpu_score_content.py) can hold the kernels to cases whose reason
is checked here: which sources tie (bit for bit, or within 1e-12 with
distinct bits), which planner branch every geometry takes, and that every
parameter override moves the oracle's answer.

The figures in the comments ("seen") are what the oracle gave when the cases
were written; the assertions are the properties, not the figures.
"""
import numpy as np
import pytest

from tests import _score_content as C

W, H = C.TIE_W, C.TIE_H


def _ties(name, params=None):
    ref = C.ref_for(name, W, H, params=params)
    t = C.totals(ref)
    near = C.near_ties(ref)
    return ref, C.exact_ties(ref), near, {t[i].hex() for i in near}


# ---- 1. content that ties ---------------------------------------------------
@pytest.mark.parametrize("name", ["flat_grey", "flat_grey40"])
def test_flat_grey_ties_bit_for_bit_beyond_the_first_scale(name):
    """seen: 12 crops share the maximum, top 26 (the second scale's second row)"""
    ref, exact, _, _ = _ties(name)
    assert len(exact) >= 2
    assert ref["top_index"] == exact[0] != 0
    _, _, xs, ys = C.scales(ref)[0]
    assert ref["top_index"] >= len(xs) * len(ys)  # past the first scale's crops


def test_flat_black_is_not_flat_to_the_edge_detector():
    """Flat black does NOT tie at the maximum: smartcrop.py's edge kernel has
    offset 1 and Pillow copies the border, so the edge map of a black image is
    0 on the border and 1 inside.  The crops that touch the left border differ
    from the inner ones; crop 0 wins alone (seen: total 2.485e-4, 3 % above the
    next) and the inner crops of the first scale lie within 1e-12 of each other
    below it, with distinct bits.  Kept as a source for what it does give:
    near-tied runners-up that must not win, and maps that are 0 almost
    everywhere."""
    ref, exact, near, _ = _ties("flat_black")
    m = ref["maps"]
    assert m[..., 0].max() == 0 and m[..., 2].max() == 0
    assert m[0, :, 1].max() == 0 and m[:, 0, 1].max() == 0 and np.all(m[1:-1, 1:-1, 1] == 1)
    assert ref["top_index"] == 0 and exact == [0] and near == [0]
    t = C.totals(ref)
    assert len({v.hex() for v in t[1:11]}) >= 2 and max(t[1:11]) - min(t[1:11]) <= 1e-12 * t[1]
    assert max(t[1:]) < t[0] * 0.999


def test_tile_near_ties_with_distinct_bits():
    """seen (seed 1): 10 crops within 1e-12 of the maximum, 5 distinct totals,
    3 of them bit-equal to the maximum, top 2 (not the first crop)"""
    ref, exact, near, bits = _ties("tile")
    assert len(near) >= 2 and len(bits) >= 2
    assert len(exact) >= 2
    assert ref["top_index"] == exact[0]


def test_flat_skin_near_ties_with_distinct_bits():
    """seen: 12 within 1e-12, 2 distinct totals, 3 bit-equal to the maximum, top 27"""
    ref, exact, near, bits = _ties("flat_skin")
    assert len(near) >= 2 and len(bits) >= 2
    assert ref["maps"][..., 0].min() > 0  # a skin colour everywhere


def test_tile_without_outside_importance_ties_exactly():
    """seen: 12 exact ties, top 26"""
    ref, exact, _, _ = _ties("tile", {"outside_importance": 0.0})
    assert len(exact) >= 2


def test_zero_weights_tie_every_crop_at_zero():
    p = {"detail_weight": 0.0, "skin_weight": 0.0, "saturation_weight": 0.0}
    for name in ("noise", "tile"):
        ref, exact, _, _ = _ties(name, p)
        assert all(v == 0.0 for v in C.totals(ref))
        assert len(exact) == len(ref["crops"]) and ref["top_index"] == 0


def test_checkers_swing_every_map_end_to_end():
    """maps are (skin, edge, saturation).  seen: checker skin 0..170, edge
    0..255, saturation 0..255, skin * edge up to 43350; checker_sat saturation *
    edge up to 65025.  The products' high bytes pass 128, so k_sc_score3's
    value - 128 planes hold both signs."""
    m = C.ref_for("checker", W, H)["maps"].astype(int)
    s, e, t = m[..., 0], m[..., 1], m[..., 2]
    assert (e.min(), e.max()) == (0, 255) and (t.min(), t.max()) == (0, 255)
    assert s.min() == 0 and s.max() >= 128
    se = s * e
    assert se.min() == 0 and (se >> 8).max() >= 128 and (se & 255).max() >= 128 and (se & 255).min() < 128
    m = C.ref_for("checker_sat", W, H)["maps"].astype(int)
    te = m[..., 2] * m[..., 1]
    assert te.min() == 0 and te.max() == 255 * 255


def test_noise_is_the_control():
    ref, exact, near, _ = _ties("noise")
    assert len(exact) == 1 and len(near) == 1


@pytest.mark.parametrize("case", C.TIE_CASES, ids=[c.name for c in C.TIE_CASES])
def test_tie_cases_plan_the_stated_kernel(case):
    ref = C.ref_for(case.source, W, H, params=case.params)
    p = C.planned(ref, W, H, 8, case.params)
    assert (p.kernel, p.groups) == (case.kernel, case.groups), p


# ---- 2./3. geometries and the planner branch they take ---------------------------
@pytest.mark.parametrize("case", C.GEO_CASES, ids=[c.name for c in C.GEO_CASES])
def test_geometry_facts_and_planned_kernel(case):
    step = dict(C.DEFAULT_OPTIONS, **case.options)["step"]
    for content in C.GEO_CONTENT:  # the crop list does not depend on the pixels
        ref = C.ref_for(content, case.W, case.H, case.tw, case.th, case.options)
        facts = [(nx, len(xs), len(ys)) for nx, _, xs, ys in C.scales(ref)]
        assert facts == case.facts
        p = C.planned(ref, case.W, case.H, step)
        assert (p.kernel, p.groups, p.why) == (case.kernel, case.groups, case.why), p


def test_geometries_cover_the_planner():
    by = {c.name: c for c in C.GEO_CASES}
    widths = {f[0] for c in C.GEO_CASES if len(c.facts) == 1 for f in c.facts}
    assert {64, 65, 128, 129} <= widths
    assert by["win64"].kernel == by["win65"].kernel == by["win128"].kernel == C.S3 and by["win129"].why == "k-steps"
    assert {f[2] for c in C.GEO_CASES for f in c.facts} >= {3, 4, 7}
    assert {f[1] for c in C.GEO_CASES for f in c.facts} >= {16, 17}
    assert {len(c.facts) for c in C.GEO_CASES} >= {1, 2, 3, 4}
    assert {dict(C.DEFAULT_OPTIONS, **c.options)["step"] for c in C.GEO_CASES} >= {1, 4, 5, 8, 16}
    n = {k: len(C.ref_for("noise", c.W, c.H, c.tw, c.th, c.options)["crops"])
         for k, c in by.items() if k.startswith("step1") or k == "whole_image"}
    assert n["step1_below"] <= C.K_SCORE_MAX_CROPS < n["step1_above"] and n["whole_image"] == 1
    assert any(c.tw > c.th for c in C.GEO_CASES) and any(c.tw < c.th for c in C.GEO_CASES)
    assert any(c.H > c.W for c in C.GEO_CASES)
    px = by["maps_lds_at"].W * by["maps_lds_at"].H, by["maps_lds_over"].W * by["maps_lds_over"].H
    assert px[0] * 4 == C.K_SCORE_LDS_MAPS < px[1] * 4
    # several cases on each kernel, k_sc_score3 with one group and with two
    kernels = [(c.kernel, c.groups) for c in C.GEO_CASES]
    for k in ((C.S3, 1), (C.S3, 2), (C.S2_LDS, 0), (C.S2_GLOBAL, 0)):
        assert kernels.count(k) >= 2, k
    assert {c.why for c in C.GEO_CASES} >= {"", "k-steps", "groups", "x origins off the 8-byte grid", "LDS"}


@pytest.mark.parametrize("name,content", C.GEO_EXTRA, ids=["-".join(e) for e in C.GEO_EXTRA])
def test_extra_flat_content_ties(name, content):
    c = {g.name: g for g in C.GEO_CASES}[name]
    ref = C.ref_for(content, c.W, c.H, c.tw, c.th, c.options)
    assert len(C.near_ties(ref)) >= 2
    if content == "flat_grey" and name != "ys4":
        assert len(C.exact_ties(ref)) >= 2


# ---- 4. parameters ---------------------------------------------------------------
@pytest.mark.parametrize("case", C.PARAM_CASES, ids=[c.name for c in C.PARAM_CASES])
def test_param_override_moves_the_oracle(case):
    moved = False
    for content in C.PARAM_CONTENT:
        base = C.ref_for(content, W, H)
        ref = C.ref_for(content, W, H, params=case.params)
        moved |= ref["top_index"] != base["top_index"] or \
            [v.hex() for v in C.totals(ref)] != [v.hex() for v in C.totals(base)]
        p = C.planned(ref, W, H, 8, case.params)
        assert p.kernel == case.kernel and (p.why == "fast_ok") == case.all_exact
    assert moved


@pytest.mark.parametrize("w,h,k,kernel", C.TUNED_CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}" for c in C.TUNED_CASES])
def test_tuned_weight_ties_two_unrelated_crops(w, h, k, kernel):
    """seen: leaders 0 to 3e-15 (relative) apart, one pair bit-equal across two
    scales; the weights are mostly negative (the bound's fabs terms)"""
    pair = C.weight_crossings(w, h)[k]
    assert pair[1] == np.nextafter(pair[0], 2.0)
    tops = []
    for wd in pair:
        ref = C.ref_for("noise", w, h, params={"detail_weight": wd})
        t = C.totals(ref)
        assert [v.hex() for v in t] == [v.hex() for v in C.totals_at(C.ref_for("noise", w, h), wd).tolist()]
        a, b = sorted(t, reverse=True)[:2]
        assert a - b <= 1e-14 * abs(a)
        assert C.planned(ref, w, h, 8).kernel == kernel
        tops.append(ref["top_index"])
    assert tops[0] != tops[1]
    # the two leaders see different pixels (noise): nothing but the weight ties them
    img = C.noise(w, h)
    wa, wb = (img[c["y"]:c["y"] + 32, c["x"]:c["x"] + 32] for c in (ref["crops"][i] for i in tops))
    assert not np.array_equal(wa, wb)


def test_tuned_weights_have_the_crossings_the_table_names():
    for w, h in {(c[0], c[1]) for c in C.TUNED_CASES}:
        assert len(C.weight_crossings(w, h)) == sum(1 for c in C.TUNED_CASES if (c[0], c[1]) == (w, h))


# ---- 5. the batch ----------------------------------------------------------------
def test_batch_prescale_is_the_identity_and_ties_are_as_stated():
    from flyimg_amd import _lib as L
    from flyimg_amd.runtime import Op, plan
    from oracle import oracle as orc

    plans = set()
    for source, w, h, t in C.BATCH:
        assert plan(w, h, Op(0, 0, L.FI_OP_SMARTCROP, L.GRAVITY["Center"], 0, t, t)) == (w, h, 3)
        ref = orc.sc_crop(C.SOURCES[source](w, h), t, t)  # the pipeline's options: prescale on
        assert ref["analyse_size"] == (w, h) and ref["prescale"] == 1.0
        assert (len(C.exact_ties(ref)) >= 2) == (source not in C.BATCH_UNTIED), (source, w, h)
        plans.add((w, h, t))
    assert len(plans) >= 3 and len(plans) < len(C.BATCH)  # shared plans next to others
