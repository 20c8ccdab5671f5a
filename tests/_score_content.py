"""Crafted analysis-resolution images, geometries and parameter sets for the
smart-crop score stage (fi_sc_score.hip, planned by plan_score_groups in
fi_sc_plan.cpp), shared by tests/test_score_content_cpu.py (which proves on
the oracle alone that every source ties, or not, the way its name says and that
every geometry lands on the planner branch it was built for) and
tests/test_gpu_score_content.py (which holds the three score kernels to the
oracle on them).

Everything runs with ``prescale = 0``: the sources are the analysed images, so
the structure that makes crops tie (flat areas, a tile whose period is the
crop step) reaches the score stage untouched.

``planned()`` restates plan_score_groups' rules on the oracle's crop list; the
case tables state the kernel each case is meant to reach and the CPU file
checks the statement against the restatement, the GPU file against the
context's counters.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

from oracle import oracle as orc

# fi_internal.h
K_SG_MAX = 2            # kSgMax: k_sc_score3 groups per image
K_SG_SLOTS = 3          # kSgSlots: y origins per group
K_SG_MAX_KS = 2         # kSgMaxKs: 64-px k-steps per window row
K_SG_PLANES = 7         # kSgPlanes
K_SCORE3_LDS = 160 * 1024 - 4608   # kScore3Lds
K_SCORE_LDS_MAPS = 112 * 1024      # kScoreLdsMaps (bytes: 28,672 px)
K_SCORE_MAX_CROPS = 1024           # kScoreMaxCrops

MFMA, VALU = "sc_score_mfma", "sc_score_valu"   # Context.stats counters
S3, S2_LDS, S2_GLOBAL = "k_sc_score3", "k_sc_score2<1>", "k_sc_score2<0>"

DEFAULT_OPTIONS = dict(max_scale=1.0, min_scale=0.9, scale_step=0.1, step=8)


# ---------------------------------------------------------------------------
# sources (H x W x 3 uint8, deterministic)
# ---------------------------------------------------------------------------
def flat(W, H, rgb):
    a = np.empty((H, W, 3), np.uint8)
    a[:] = np.asarray(rgb, np.uint8)
    return a


def flat_grey(W=200, H=112):
    return flat(W, H, (128, 128, 128))


def flat_grey40(W=200, H=112):
    return flat(W, H, (40, 40, 40))


def flat_black(W=200, H=112):
    """not flat to the edge detector (its kernel has offset 1, the border is
    copied: 0 on the border, 1 inside): one clear winner, near-tied runners-up"""
    return flat(W, H, (0, 0, 0))


SKIN = (200, 150, 120)
BLUE = (0, 0, 255)


def flat_skin(W=200, H=112):
    return flat(W, H, SKIN)


TILE_SEED = 1


def tile(W=200, H=112, seed=TILE_SEED, period=8):
    """a period x period random tile repeated: with the period equal to the
    crop step every crop of a scale that is not cut by the image's edge sees
    the same pixels under the same importance weights"""
    t = np.random.default_rng(seed).integers(0, 256, (period, period, 3), dtype=np.uint8)
    reps = ((H + period - 1) // period, (W + period - 1) // period, 1)
    return np.ascontiguousarray(np.tile(t, reps)[:H, :W])


def _checker(W, H, even, odd):
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.empty((H, W, 3), np.uint8)
    m = ((xx + yy) & 1).astype(bool)
    a[~m] = even
    a[m] = odd
    return a


def checker(W=200, H=112):
    """1-px checker of a skin colour against saturated blue: the edge, skin and
    saturation maps each hold 0 and their maximum, and skin * edge swings from
    0 to beyond 2^15 (k_sc_score3's signed-byte planes at both ends)"""
    return _checker(W, H, SKIN, BLUE)


ORANGE = (255, 180, 0)


def checker_sat(W=200, H=112):
    """1-px checker of a bright saturated colour against black: saturation *
    edge swings from 0 to 255 * 255"""
    return _checker(W, H, ORANGE, (0, 0, 0))


def noise(W=200, H=112, seed=11):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


SOURCES = {"flat_grey": flat_grey, "flat_grey40": flat_grey40, "flat_black": flat_black, "flat_skin": flat_skin,
           "tile": tile,
           "checker": checker, "checker_sat": checker_sat, "noise": noise}


# ---------------------------------------------------------------------------
# the oracle and what the planner does with its crop list
# ---------------------------------------------------------------------------
def oracle(img, tw=100, th=100, options=None, params=None):
    o = dict(DEFAULT_OPTIONS, **(options or {}))
    p = orc.default_params(**params) if params else None
    return orc.sc_crop(img, tw, th, prescale=False, params=p, **o)


_REFS = {}


def ref_for(source, W, H, tw=100, th=100, options=None, params=None):
    """the oracle's result for a named source, computed once (read-only)"""
    key = (source, W, H, tw, th, tuple(sorted((options or {}).items())), tuple(sorted((params or {}).items())))
    if key not in _REFS:
        _REFS[key] = oracle(SOURCES[source](W, H), tw, th, options, params)
    return _REFS[key]


def totals(ref):
    return [c["score"]["total"] for c in ref["crops"]]


def exact_ties(ref):
    """indices of the crops whose total equals the maximum bit for bit"""
    t = totals(ref)
    m = max(t)
    return [i for i, v in enumerate(t) if v.hex() == m.hex()]


def near_ties(ref, rel=1e-12):
    """indices of the crops within `rel` (relative) of the maximum"""
    t = totals(ref)
    m = max(t)
    return [i for i, v in enumerate(t) if abs(v - m) <= rel * max(abs(m), 1e-300)]


def scales(ref):
    """per scale, in the order of the crop list: (window width px, window height
    px, sorted distinct x origins, sorted distinct y origins)"""
    out = []
    for c in ref["crops"]:
        k = (c["fw"], c["fh"])
        if not out or out[-1][0] != k:
            assert all(o[0] != k for o in out), "crops() lists a scale's crops together"
            out.append((k, set(), set()))
        out[-1][1].add(c["x"])
        out[-1][2].add(c["y"])
    return [(math.ceil(k[0]), math.ceil(k[1]), sorted(xs), sorted(ys)) for k, xs, ys in out]


Planned = namedtuple("Planned", "counter kernel groups why")


def planned(ref, W, H, step, params=None):
    """plan_score_groups + add_sc_launches restated: which score kernel an image
    with this crop list runs on the default context, with how many k_sc_score3
    groups, and the first rule that sends it to k_sc_score2."""
    params = params or {}
    valu = S2_LDS if W * H * 4 <= K_SCORE_LDS_MAPS else S2_GLOBAL

    def no(why):
        return Planned(VALU, valu, 0, why)

    if params.get("skin_bias", 0.01) < 0 or params.get("saturation_bias", 0.2) < 0:
        return no("fast_ok")
    groups, tail = 0, 0
    for nx, ny, xs, ys in scales(ref):
        if nx * ny >= 1 << 17:
            return no("window pixels")
        if any(b - a != step for a, b in zip(ys, ys[1:])):
            return no("y origins not a step apart")
        if any(x % 8 for x in xs):
            return no("x origins off the 8-byte grid")
        ks = (nx + 63) // 64
        if ks > K_SG_MAX_KS:
            return no("k-steps")
        for xa in range(0, len(xs), 16):
            last = xs[min(xa + 16, len(xs)) - 1]
            tail = max(tail, last + 64 * ks)
            groups += (len(ys) + K_SG_SLOTS - 1) // K_SG_SLOTS
    if groups > K_SG_MAX:
        return no("groups")
    pitch = (W + 7) & ~7
    lds = max(K_SG_PLANES * H * pitch + max(0, tail - pitch) + 16, W * H * 4, groups * K_SG_PLANES * 1024)
    if lds > K_SCORE3_LDS:
        return no("LDS")
    return Planned(MFMA, S3, groups, "")


# ---------------------------------------------------------------------------
# 1. content that ties (and a control that does not), on TIE_W x TIE_H with the
#    default options; kernel / groups: what planned() must say
# ---------------------------------------------------------------------------
TieCase = namedtuple("TieCase", "name source params kernel groups")
TIE_W, TIE_H = 200, 112   # two scales, one group each: 12 x 1 and 13 x 2 origins
TIE_CASES = [
    TieCase("flat_grey", "flat_grey", {}, S3, 2),
    TieCase("flat_grey40", "flat_grey40", {}, S3, 2),
    TieCase("flat_black", "flat_black", {}, S3, 2),
    TieCase("tile", "tile", {}, S3, 2),
    TieCase("flat_skin", "flat_skin", {}, S3, 2),
    TieCase("tile_oi0", "tile", {"outside_importance": 0.0}, S3, 2),
    TieCase("noise_w0", "noise", {"detail_weight": 0.0, "skin_weight": 0.0, "saturation_weight": 0.0}, S3, 2),
    TieCase("checker", "checker", {}, S3, 2),
    TieCase("checker_sat", "checker_sat", {}, S3, 2),
    TieCase("noise", "noise", {}, S3, 2),
]

# ---------------------------------------------------------------------------
# 2. geometries.  facts: per scale (window width, distinct x origins, distinct
#    y origins); kernel / groups / why: what planned() must say
# ---------------------------------------------------------------------------
GeoCase = namedtuple("GeoCase", "name W H tw th options facts kernel groups why")


def _g(name, W, H, tw, th, options, facts, kernel, groups=0, why=""):
    return GeoCase(name, W, H, tw, th, options, facts, kernel, groups, why)


ONE = dict(max_scale=0.9, min_scale=0.9)
GEO_CASES = [
    # window widths: one k-step, two, and one past kSgMaxKs (a target larger
    # than the image: one scale of the whole height)
    _g("win64", 120, 64, 100, 100, {}, [(64, 8, 1)], S3, 1),
    _g("win65", 121, 65, 100, 100, {}, [(65, 8, 1)], S3, 1),
    _g("win128", 160, 128, 200, 200, {}, [(128, 5, 1)], S3, 1),
    _g("win129", 161, 129, 200, 200, {}, [(129, 5, 1)], S2_LDS, 0, "k-steps"),
    # y origins in a scale: a full slot chunk, a chunk of one after it, three chunks
    _g("ys3", 64, 80, 100, 100, {}, [(64, 1, 3)], S3, 1),
    _g("ys4", 64, 88, 100, 100, {}, [(64, 1, 4)], S3, 2),
    _g("ys7", 64, 112, 100, 100, {}, [(64, 1, 7)], S2_LDS, 0, "groups"),
    # x origins in a scale: a full chunk of 16 M rows, and a 17th in a group of its own
    _g("xs16", 184, 64, 100, 100, {}, [(64, 16, 1)], S3, 1),
    _g("xs17", 192, 64, 100, 100, {}, [(64, 17, 1)], S3, 2),
    # scales
    _g("one_scale", 200, 112, 100, 100, ONE, [(101, 13, 2)], S3, 1),
    _g("three_scales", 200, 112, 100, 100, dict(min_scale=0.8),
       [(112, 12, 1), (101, 13, 2), (90, 14, 3)], S2_LDS, 0, "groups"),
    _g("three_scales_small", 96, 80, 50, 50, dict(max_scale=0.9, min_scale=0.7),
       [(72, 4, 2), (64, 5, 3), (56, 6, 4)], S2_LDS, 0, "groups"),
    _g("scale_step15", 200, 112, 70, 70, dict(min_scale=0.7, scale_step=0.15),
       [(112, 12, 1), (96, 14, 3), (79, 16, 5), (62, 18, 7)], S2_LDS, 0, "groups"),
    # steps
    _g("step4", 200, 112, 100, 100, dict(step=4), [(112, 23, 1), (101, 25, 3)], S2_LDS, 0,
       "x origins off the 8-byte grid"),
    _g("step5", 200, 112, 100, 100, dict(step=5), [(112, 18, 1), (101, 20, 3)], S2_LDS, 0,
       "x origins off the 8-byte grid"),
    _g("step16", 200, 112, 100, 100, dict(step=16), [(112, 6, 1), (101, 7, 1)], S3, 2),
    _g("step16_slots", 120, 150, 100, 100, dict(step=16), [(120, 1, 2), (108, 1, 3)], S3, 2),
    _g("step1_below", 180, 120, 100, 100, dict(step=1), [(120, 61, 1), (108, 73, 13)], S2_LDS, 0,
       "x origins off the 8-byte grid"),
    _g("step1_above", 184, 120, 100, 100, dict(step=1), [(120, 65, 1), (108, 77, 13)], S2_LDS, 0,
       "x origins off the 8-byte grid"),
    # non-square targets both ways, portrait sources
    _g("wide_target", 128, 96, 160, 90, {}, [(128, 1, 4)], S3, 2),
    _g("tall_target", 96, 128, 90, 160, {}, [(72, 4, 1)], S3, 1),
    _g("wide_target_two_scales", 200, 112, 160, 90, {}, [(199, 1, 1), (180, 3, 2)], S2_LDS, 0, "k-steps"),
    _g("tall_target_portrait", 112, 200, 90, 160, {}, [(112, 1, 1), (101, 2, 3)], S3, 2),
    _g("portrait", 112, 200, 100, 100, {}, [(112, 1, 12), (101, 2, 13)], S2_LDS, 0, "groups"),
    # the LDS caps: k_sc_score3's planes, k_sc_score2's maps (28,672 px)
    _g("s3_lds_over", 208, 112, 100, 100, {}, [(112, 13, 1), (101, 14, 2)], S2_LDS, 0, "LDS"),
    _g("maps_lds_at", 224, 128, 100, 100, {}, [(128, 13, 1), (116, 14, 2)], S2_LDS, 0, "LDS"),
    _g("maps_lds_over", 225, 128, 100, 100, {}, [(128, 13, 1), (116, 14, 2)], S2_GLOBAL, 0, "LDS"),
    _g("big", 240, 160, 100, 100, {}, [(160, 11, 1), (144, 13, 3)], S2_GLOBAL, 0, "k-steps"),
    # a crop as large as the whole image
    _g("whole_image", 96, 96, 100, 100, {}, [(96, 1, 1)], S3, 1),
]
GEO_CONTENT = ("noise", "tile")
# flat content (every inner crop of a scale ties bit for bit) where the
# candidate list is long: k_sc_score2 from global maps, and its form for more
# crops than kScoreMaxCrops, which keeps the candidate marks in global memory
GEO_EXTRA = [("big", "flat_grey"), ("maps_lds_at", "flat_grey"), ("step1_below", "flat_grey"),
             ("step1_above", "flat_grey"), ("portrait", "flat_skin"), ("xs17", "flat_grey"), ("ys4", "flat_grey")]

# ---------------------------------------------------------------------------
# 4. parameter overrides (on TIE_W x TIE_H, default options)
# ---------------------------------------------------------------------------
ParamCase = namedtuple("ParamCase", "name params kernel all_exact")
PARAM_CASES = [
    ParamCase("no_thirds", {"rule_of_thirds": 0}, S3, False),
    ParamCase("oi_0", {"outside_importance": 0.0}, S3, False),
    ParamCase("oi_pos", {"outside_importance": 0.75}, S3, False),
    ParamCase("oi_neg2", {"outside_importance": -2.0}, S3, False),
    ParamCase("neg_weights", {"skin_weight": -1.8, "detail_weight": -0.2}, S3, False),
    ParamCase("edge", {"edge_radius": 0.1, "edge_weight": 5.0}, S3, False),
    ParamCase("bias_0", {"skin_bias": 0.0, "saturation_bias": 0.0}, S3, False),
    ParamCase("skin_bias_neg", {"skin_bias": -0.01}, S2_LDS, True),   # fast_ok false: every crop re-scored
    ParamCase("weights_0", {"detail_weight": 0.0, "skin_weight": 0.0, "saturation_weight": 0.0}, S3, False),
]
PARAM_CONTENT = ("tile", "noise")

# ---------------------------------------------------------------------------
# 4b. two unrelated crops made to tie by a tuned detail_weight.  The tiles and
#     flat images tie crops that are translates of each other: their fast
#     totals are equal bit for bit whatever the bound, so only the re-score and
#     the first-maximum rule are on trial there.  Here the total
#     (detail * wd + skin * ws + saturation * wt) / area of every crop is a line
#     in wd; where the lead passes from one crop of a noise image to another
#     (another position, often another scale) a bisection down to two adjacent
#     doubles gives a weight on either side of the crossing: the two leaders are
#     a few ulps apart, their fast-pass errors are unrelated, and the top crop
#     differs between the two weights.
# ---------------------------------------------------------------------------
def _lines(ref):
    cr = ref["crops"]
    return (np.array([c["score"]["detail"] for c in cr]), np.array([c["score"]["skin"] for c in cr]),
            np.array([c["score"]["saturation"] for c in cr]), np.array([c["fw"] * c["fh"] for c in cr]))


def totals_at(ref, wd, ws=1.8, wt=0.3):
    """smartcrop.py's total of every crop of `ref` at another detail_weight
    (the same operations in the same order, so the same bits)"""
    d, s, t, a = _lines(ref)
    return (d * wd + s * ws + t * wt) / a


_CROSSINGS = {}


def weight_crossings(W, H, lo=-2.0, hi=2.0, n=400):
    """[(wd_a, wd_b)]: adjacent doubles with different top crops, one pair per
    change of the top crop of noise(W, H) on a grid of n steps over [lo, hi]"""
    if (W, H) not in _CROSSINGS:
        ref = ref_for("noise", W, H)

        def top(w):
            return int(np.argmax(totals_at(ref, w)))

        grid = np.linspace(lo, hi, n + 1)
        out = []
        for a, b in zip(grid, grid[1:]):
            a, b = float(a), float(b)
            ta = top(a)
            if ta == top(b):
                continue
            while True:
                mid = (a + b) / 2
                if not a < mid < b:
                    break
                if top(mid) == ta:
                    a = mid
                else:
                    b = mid
            out.append((a, b))
        _CROSSINGS[(W, H)] = out
    return _CROSSINGS[(W, H)]


# (W, H, crossing index, kernel): seen 4, 2 and 3 crossings
TUNED_CASES = [(200, 112, k, S3) for k in range(4)] + [(224, 128, k, S2_LDS) for k in range(2)] + \
              [(240, 160, k, S2_GLOBAL) for k in range(3)]

# ---------------------------------------------------------------------------
# 5. a batch through Context.process: default options (prescale on), so the
#    smart-crop target is chosen for the prescale to be the identity
#    (asserted by the CPU file): (source, W, H, smart-crop target)
# ---------------------------------------------------------------------------
BATCH = [
    ("flat_grey", 200, 112, 104),
    ("noise", 200, 112, 104),
    ("tile", 200, 112, 104),
    ("tile", 200, 112, 112),
    ("flat_skin", 200, 112, 104),
    ("noise", 160, 128, 128),
    ("flat_grey", 240, 160, 150),
    ("noise", 240, 160, 150),
    ("flat_grey", 160, 128, 128),
    ("noise", 64, 88, 64),
    ("flat_black", 200, 112, 104),
]
BATCH_UNTIED = ("noise", "flat_black")   # every other source's maximum is shared bit for bit
