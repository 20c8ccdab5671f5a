"""GPU parity on adversarial pixel content (tests/_adversarial.py): the
resample kernels (k_rs_vr, k_rs_vm, k_rs_hv, the generic two-pass kernels,
k_rs4_*), the smartcrop prescale routes and k_conv on full-swing checkers,
1-px stripes, impulses on every block and strip seam, flats at both ends of
the range and full-range noise -- content on which the saturation between
the two passes, the p - 128 signed-byte entry, the hi / lo Q16 byte planes at
0x0000 and 0xFFFF, the border and seam taps and pil_clip8 all decide the
result (tests/test_adversarial_content_cpu.py proves that on the oracle
alone).  The geometry-varying suites (test_gpu_parity.py, test_gpu_vr.py)
feed smooth content, on which none of that code matters.

Tolerances are the project's stated ones: +-1 LSB of the oracle on every
pixel for the resamples (flats: exact), bit-exact for smartcrop and k_conv.
Exact-match fractions are logged (FI_EXACT_LOG), not asserted: the floors of
the smooth suites were measured on smooth content."""
import functools

import numpy as np
import pytest

from flyimg_amd import _lib as L
from flyimg_amd.runtime import Context, Op
from oracle import oracle as orc
from tests import _adversarial as A
from tests.test_gpu_parity import (CONV_CASES, EXPECTED_SC, PATHS, SC_PATHS, _context_with, _log_exact, _opts,
                                   _oracle_flags)

pytestmark = pytest.mark.gpu

F = L
RC = {c.name: c for c in A.RESAMPLE_CASES}


def _op(case):
    f = F.FI_OP_RESIZE if case.op == "resize" else F.FI_OP_THUMBNAIL
    f |= F.FI_GEOM_SHRINK_ONLY if case.op != "enlarge" else 0
    f |= (F.FI_GEOM_FILL | F.FI_OP_EXTENT) if case.fill else 0
    f |= F.FI_OP_GRAY if case.gray else 0
    f |= F.FI_OP_ROTATE if case.rot else 0
    return Op(case.tw, case.th, f, L.GRAVITY["Center"], case.rot)


@functools.lru_cache(maxsize=None)
def _source(name, kind, band=False):
    a = A.content(RC[name], kind, band)
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def _oracle(name, kind, band=False):
    """the oracle's output of a case's content, computed once per module"""
    op = _op(RC[name])
    src = A.flat(RC[name].W, RC[name].H, 128) if kind == "flat" else _source(name, kind, band)
    ref = orc.im_convert(src, op.target_w, op.target_h, _oracle_flags(op.flags), gravity=op.gravity, rotate=op.rotate)
    ref.flags.writeable = False
    return ref


def _expected_path(path_name, case):
    """the fi_kernel_stats counter of the kernel the path names for the case"""
    if path_name == "generic":
        return "path_generic_h" if case.hfirst else "path_generic_v"
    if case.cls == "hv":
        return "path_hv"
    return "path_vr" if case.cls == "vr" and path_name != "vm" else "path_vm"


_COUNTERS = ("path_vr", "path_vm", "path_hv", "path_generic_v", "path_generic_h")


def _run(ctx, path_name, case, srcs):
    """process `srcs` in one batch on the kernel the path names (asserted)"""
    want = _expected_path(path_name, case)
    before = {k: ctx.stats(k)[1] for k in _COUNTERS}
    outs, recs, rc = ctx.process(list(srcs), [_op(case)] * len(srcs))
    assert rc == 0 and all(r.status == 0 for r in recs), L.lib().fi_last_error()
    ran = {k: ctx.stats(k)[1] - before[k] for k in _COUNTERS}
    assert ran[want] == len(srcs) and sum(ran.values()) == len(srcs), (want, ran)
    return outs


def _within_one(gpu, ref, name):
    assert gpu is not None and gpu.shape == ref.shape, (name, None if gpu is None else gpu.shape, ref.shape)
    d = np.abs(gpu.astype(np.int16) - ref.astype(np.int16))
    exact = float((d == 0).mean())
    _log_exact(name, exact)  # recorded, not asserted
    assert d.max() <= 1, f"{name}: max |diff| {d.max()} on {int((d > 1).sum())} samples (exact {exact:.5f})"
    return exact


@pytest.fixture(scope="module", params=sorted(PATHS))
def rctx(request):
    c = _context_with(PATHS[request.param])
    c.path_name = request.param
    yield c
    c.close()


@pytest.fixture(scope="module")
def pair():
    vr, vm = _context_with(PATHS["vr"]), _context_with(PATHS["vm"])
    yield vr, vm
    vr.close()
    vm.close()


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


# --- resample: every content on every geometry on every path --------------------
@pytest.mark.parametrize("name", A.CASE_IDS)
def test_flats_stay_flat(rctx, name):
    """the quantised weight rows sum to exactly 2^shift: a flat source gives the
    same flat, at both ends of the range and around the p - 128 sign change"""
    case = RC[name]
    shape_ref = _oracle(name, "flat")
    outs = _run(rctx, rctx.path_name, case, [A.flat(case.W, case.H, v) for v in A.FLAT_VALUES])
    for v, out in zip(A.FLAT_VALUES, outs):
        assert out.shape == shape_ref.shape
        assert np.array_equal(out, np.full_like(shape_ref, v)), (name, v, np.unique(out))


@pytest.mark.parametrize("kind", A.CONTENTS)
@pytest.mark.parametrize("name", A.CASE_IDS)
def test_content_within_one_lsb_of_oracle(rctx, name, kind):
    case = RC[name]
    out = _run(rctx, rctx.path_name, case, [_source(name, kind)])[0]
    _within_one(out, _oracle(name, kind), f"{name} {kind} [{rctx.path_name}]")


VFIRST = [c.name for c in A.RESAMPLE_CASES if not c.hfirst]


@pytest.mark.parametrize("name", VFIRST)
def test_vr_equals_vm_on_every_pattern(pair, name):
    """an image's bytes do not depend on which of k_rs_vr / k_rs_vm its batch
    took (test_gpu_vr.py checks this on smooth content)"""
    vr, vm = pair
    case = RC[name]
    srcs = [_source(name, k) for k in A.CONTENTS] + [A.flat(case.W, case.H, v) for v in A.FLAT_VALUES]
    a = _run(vr, "vr", case, srcs)
    b = _run(vm, "vm", case, srcs)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), f"{name} source {k}: {int((x != y).sum())} bytes differ"


BAND = [(c.name, k) for c in A.RESAMPLE_CASES if c.band_block is not None for k in A.band_contents(c)]


@pytest.mark.parametrize("name,kind", BAND, ids=[f"{n}-{k}" for n, k in BAND])
def test_boundary_band(pair, name, kind):
    """k_rs_vr's Q16 result is proven within E Q16 units of the oracle's for
    all inputs (tests/native/vr_quant_bound.cpp; E per geometry in
    A.BAND_E): wherever the oracle's Q16 value moved by +-E still maps to the
    same byte, the byte must be the oracle's -- on both kernels (k_rs_vm
    carries the same weights).  The CPU file caps the excluded share at 30 %."""
    case = RC[name]
    src = _source(name, kind, True)
    ow, oh = orc.im_meta_geometry(case.W, case.H, case.tw, case.th, case.fill, case.op != "enlarge")
    q = orc.im_resize_q16(src, ow, oh, thumbnail=case.op != "resize")
    ref = A.q16_to_u8(q)
    inside = A.band_mask(q, A.BAND_E[name])
    for path_name, c in zip(("vr", "vm"), pair):
        out = _run(c, path_name, case, [src])[0]
        assert out.shape == ref.shape
        bad = inside & (out != ref)
        assert not bad.any(), f"{name} {kind} [{path_name}]: {int(bad.sum())} samples off inside the band"


# --- RGBA (k_rs4_*) --------------------------------------------------------------
RGBA_GEO = [
    # (name, W, H, rw, rh, oracle flags, rotate, checker side ~2.5 / factor)
    ("fill_extent_640x480_150x150", 640, 480, 150, 150, orc.FLAG_THUMBNAIL | orc.FLAG_FILL | orc.FLAG_EXTENT, 0, 8),
    ("hfirst_900x300_w120", 900, 300, 120, 0, orc.FLAG_THUMBNAIL | orc.FLAG_SHRINK, 0, 19),
    ("resize_enlarge_120x90_w300", 120, 90, 300, 0, 0, 0, 2),
    ("gray_alpha_rot90_640x480_w160", 640, 480, 160, 0, orc.FLAG_THUMBNAIL | orc.FLAG_GRAY | orc.FLAG_ROTATE, 90, 10),
]
RGBA_KINDS = [n for n, _ in A.rgba_sources(4, 4, 2)]


@functools.lru_cache(maxsize=None)
def _rgba_sources(W, H, b):
    return dict(A.rgba_sources(W, H, b))


@pytest.mark.parametrize("kind", RGBA_KINDS)
@pytest.mark.parametrize("geo", RGBA_GEO, ids=[g[0] for g in RGBA_GEO])
def test_rgba_within_one_lsb_of_oracle(ctx, geo, kind):
    """matte sources on the alpha-weighted passes: +-1 LSB of the oracle on
    every sample; opaque stays opaque, transparent stays transparent (colour
    through PerceptibleReciprocal of a zero alpha sum)"""
    gname, W, H, rw, rh, flags, rot, b = geo
    src = _rgba_sources(W, H, b)[kind]
    ref = orc.im_convert(src, rw, rh, flags, 5, rot)
    f = F.FI_OP_THUMBNAIL if flags & orc.FLAG_THUMBNAIL else F.FI_OP_RESIZE
    f |= F.FI_GEOM_FILL if flags & orc.FLAG_FILL else 0
    f |= F.FI_GEOM_SHRINK_ONLY if flags & orc.FLAG_SHRINK else 0
    f |= F.FI_OP_EXTENT if flags & orc.FLAG_EXTENT else 0
    f |= F.FI_OP_GRAY if flags & orc.FLAG_GRAY else 0
    f |= F.FI_OP_ROTATE if flags & orc.FLAG_ROTATE else 0
    before = ctx.stats("path_generic_v")[1] + ctx.stats("path_generic_h")[1]
    outs, recs, rc = ctx.process([src], [Op(rw, rh, f, L.GRAVITY["Center"], rot)])
    L.check(rc)
    assert recs[0].status == 0
    assert ctx.stats("path_generic_v")[1] + ctx.stats("path_generic_h")[1] == before + 1  # the k_rs4_* passes
    out = outs[0]
    assert out.shape[-1] == (2 if flags & orc.FLAG_GRAY else 4)
    _within_one(out, ref, f"rgba {gname} {kind}")
    if kind.endswith("_a255"):
        assert (out[..., -1] == 255).all()
    if kind.endswith("_a0"):
        assert (out[..., -1] == 0).all()


# --- smartcrop prescale routes -----------------------------------------------------
@pytest.fixture(scope="module", params=sorted(SC_PATHS))
def sctx(request):
    c = _context_with(SC_PATHS[request.param])
    c.path_name = request.param
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _sc_case(W, H, gray, kind):
    src = A.sc_source(W, H, gray, kind)
    return src, orc.sc_crop(src, 100, 100)


@pytest.mark.parametrize("kind", A.SC_CONTENTS)
@pytest.mark.parametrize("W,H,gray", A.SC_SIZES, ids=[f"{w}x{h}{'-gray' if g else ''}" for w, h, g in A.SC_SIZES])
def test_smartcrop_bit_exact(sctx, W, H, gray, kind):
    """prescale (pil_clip8 clipping both ways on the checkers) + maps + scores
    on every prescale route: the prescaled image and the maps are the
    oracle's byte for byte, every crop's four scores bit for bit, and the
    route's own kernel ran"""
    src, ref = _sc_case(W, H, gray, kind)
    names = ("sc_path_cx", "sc_path_fd", "sc_path_fz")
    before = {k: sctx.stats(k)[1] for k in names}
    r = sctx.smartcrop_ex(src, 100, 100, options=_opts(True), want_images=True)
    ran = {k: sctx.stats(k)[1] - before[k] for k in names}
    want = EXPECTED_SC[sctx.path_name]
    if want is not None:
        assert ran[want] == 1 and sum(ran.values()) == 1, ran
    else:
        assert sum(ran.values()) == 0, ran
    assert tuple(r["analyse_size"]) == tuple(ref["analyse_size"]) and r["prescale"].hex() == ref["prescale"].hex()
    assert np.array_equal(r["prescaled"], ref["prescaled"]), int((r["prescaled"] != ref["prescaled"]).sum())
    assert np.array_equal(r["maps"], ref["maps"]), int((r["maps"] != ref["maps"]).sum())
    assert r["n"] == len(ref["crops"]) and r["top_index"] == ref["top_index"]
    for c, g in zip(r["crops"], ref["crops"]):
        assert [c.x, c.y, c.width, c.height] == [g["x"], g["y"], g["width"], g["height"]]
        assert [c.detail.hex(), c.saturation.hex(), c.skin.hex(), c.total.hex()] == \
            [g["score"][k].hex() for k in ("detail", "saturation", "skin", "total")]


# --- forwarded convolutions (k_conv) --------------------------------------------------
@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_convolve_bit_exact(ctx, case, ch):
    """-unsharp / -sharpen / -blur on Q16 content that drives ClampToQuantum
    below 0 and above 65535, and on images narrower and lower than the kernel
    (every tap an edge tap): the oracle's bytes, bit for bit"""
    _, conv, ops = case
    for name, q in A.conv_sources(ch):
        got = ctx.convolve_q16(q, conv, ops)
        ref = orc.im_convolve_q16(q, conv, ops)
        assert got.shape == ref.shape and np.array_equal(got, ref), (case[0], ch, name, int((got != ref).sum()))
