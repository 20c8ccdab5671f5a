"""k_rs_vr (the persistent block-major resample, fi_vr.hip) on every geometry
class it takes: the path actually ran (its image counter rose by the batch),
the output is bit-identical to k_rs_vm's (which carries k_rs_vr's two-limb
weights scaled to 2^22, fi_plan_mfma.cpp axis_q22 -- so an image's pixels do not
depend on which kernel its batch took), and within +-1 LSB / >= 99.5 % exact (99.9 % on the BASELINE geometries) of
the oracle (ImageProcessor.php:86 -thumbnail / -resize, IM's VerticalFilter
then HorizontalFilter)."""
import functools

import numpy as np
import pytest

from flyimg_amd import _lib as L
from flyimg_amd.processor import ImageProcessor, OptionsBag
from flyimg_amd.synth import synth_rgb as _synth_rgb
from oracle import oracle as orc
from tests.test_gpu_parity import MIN_EXACT, MIN_EXACT_BASELINE, _context_with, _log_exact, _oracle_flags

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=24)
def synth_rgb(W, H, seed):
    """the seeded synthetic source, generated once per module (the role-split
    parametrizations reuse the 24 MP inputs; the kernels only read them)"""
    a = _synth_rgb(W, H, seed)
    a.flags.writeable = False
    return a

CASES = [
    # (W, H, options, images)
    (1920, 1080, "w_500", 3),
    (1920, 1080, "w_500", 40),
    (3840, 2160, "w_512,h_512,c_1", 2),
    (6000, 4000, "w_400,h_400,c_1,r_90,clsp_Gray", 2),
    (1024, 768, "w_200,h_200,c_1,r_180", 2),
    (1200, 900, "w_300,r_270", 2),
    (800, 600, "w_250,clsp_Gray", 2),
    (333, 517, "w_97", 4),
    (4000, 3000, "w_150", 2),  # sampled rows 5.33 apart: uneven, streamed from the row list
    (3000, 2000, "w_300,h_250,c_1", 3),  # cfg1: 1250 of 2000 rows at gaps of 1 and 2
    (3840, 2160, "w_512,h_512,c_1", 300),
    (1920, 1080, "w_500", 300),
    (6000, 4000, "w_400,h_400,c_1,r_90,clsp_Gray", 12),
    (640, 480, "w_320", 7),  # 1/2: 64-px strips would carry four 16-px blocks; built at 48 px for k_rs_vr
]


# k_rs_vm's class (FI_VR_NARROW=0 puts the 1/2 case back there: test_narrow_strips_switch)
NOT_VR = set()


@pytest.fixture(scope="module")
def pair():
    vr = _context_with({"FI_VR_RS": "1", "FI_FORCE_GENERIC": "0"})
    vm = _context_with({"FI_VR_RS": "0", "FI_FORCE_GENERIC": "0"})
    yield vr, vm
    vr.close()
    vm.close()


def _close(a, b, name, min_same):
    assert a is not None and b is not None and a.shape == b.shape, name
    d = np.abs(a.astype(np.int16) - b.astype(np.int16))
    same = float((d == 0).mean())
    _log_exact(name, same)  # record only; the two assertions below still decide
    assert d.max() <= 1, f"{name}: max |diff| {d.max()}"
    assert same >= min_same, f"{name}: identical fraction {same:.5f}"
    return same


def _oracle(src, op):
    return orc.im_convert(src, op.target_w, op.target_h, _oracle_flags(op.flags), gravity=op.gravity, rotate=op.rotate)


@pytest.mark.parametrize("W,H,opts,n", CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}-x{c[3]}" for c in CASES])
def test_vr_takes_the_class_and_matches(pair, W, H, opts, n):
    vr, vm = pair
    op = ImageProcessor(OptionsBag(opts), W, H).to_op()
    base = [synth_rgb(W, H, 77 + k) for k in range(min(n, 4))]
    srcs = [base[k % len(base)] for k in range(n)]
    path = "path_vr" if (W, H, opts) not in NOT_VR else "path_vm"
    before = vr.stats(path)[1]
    ob, rb, rcb = vr.process(srcs, [op] * n)
    assert rcb == 0 and all(r.status == 0 for r in rb), L.lib().fi_last_error()
    assert vr.stats(path)[1] == before + n  # no silent fallback to another kernel
    assert vr.stats("vr_ablation")[1] == 0  # production kernel (no FI_VR_VARIANT ablation)
    oa, ra, rca = vm.process(srcs[:len(base)], [op] * len(base))
    assert rca == 0
    for k in range(len(base)):
        assert np.array_equal(ob[k], oa[k]), f"{opts} image {k}: k_rs_vr != k_rs_vm"
        for j in range(k, n, len(base)):  # repeated sources give identical outputs
            assert np.array_equal(ob[j], ob[k])
    if W * H <= 4_000_000:
        baseline = (W, H, opts) in {(1920, 1080, "w_500"), (3000, 2000, "w_300,h_250,c_1")}
        _close(ob[0], _oracle(base[0], op), f"{opts} vs oracle", MIN_EXACT_BASELINE if baseline else MIN_EXACT)


def test_vr_mixed_batch(pair):
    """one launch with several vertical tables: 8-bit and Q16 (gray / rotated)
    output tiles, unequal tile costs (1080p, 4K, small images), checked image
    by image against the oracle and against k_rs_vm"""
    vr, vm = pair
    geo = [(1920, 1080, "w_500"), (3840, 2160, "w_512,h_512,c_1"), (800, 600, "w_250,clsp_Gray"),
           (1200, 900, "w_300,r_270"), (333, 517, "w_97"), (1024, 768, "w_200,h_200,c_1,r_180")]
    srcs, ops = [], []
    for k in range(12):
        W, H, opts = geo[k % len(geo)]
        srcs.append(synth_rgb(W, H, 300 + k))
        ops.append(ImageProcessor(OptionsBag(opts), W, H).to_op())
    before = vr.stats("path_vr")[1]
    ob, rb, rcb = vr.process(srcs, ops)
    assert rcb == 0 and all(r.status == 0 for r in rb)
    assert vr.stats("path_vr")[1] == before + len(srcs)
    oa, _, rca = vm.process(srcs, ops)
    assert rca == 0
    for k in range(len(srcs)):
        assert np.array_equal(ob[k], oa[k]), f"mixed {k}: k_rs_vr != k_rs_vm"
        if srcs[k].shape[0] * srcs[k].shape[1] <= 4_000_000:
            _close(ob[k], _oracle(srcs[k], ops[k]), f"mixed {k} vs oracle", MIN_EXACT)


def test_output_independent_of_cobatched_images(pair):
    """an image's pixels depend only on the image -- alone its batch
    runs k_rs_vr; inside a batch of more vertical geometries than a context's
    FI_VR_MAX_CLASSES (8 here) the batch takes k_rs_vm; the bytes are the same."""
    vr = _context_with({"FI_VR_RS": "1", "FI_FORCE_GENERIC": "0", "FI_VR_MAX_CLASSES": "8"})
    W, H, opts = 1920, 1080, "w_500,clsp_Gray"
    src = synth_rgb(W, H, 4242)
    op = ImageProcessor(OptionsBag(opts), W, H).to_op()
    before = vr.stats("path_vr")[1]
    alone, _, rc = vr.process([src], [op])
    assert rc == 0 and vr.stats("path_vr")[1] == before + 1
    srcs, ops = [src], [op]
    for k, (w, h) in enumerate([(1000, 700), (1100, 800), (1300, 900), (1500, 1000), (1700, 1100),
                                (900, 1200), (1234, 987), (2000, 1500), (777, 555), (1600, 1300)]):
        srcs.append(synth_rgb(w, h, 500 + k))
        ops.append(ImageProcessor(OptionsBag("w_%d" % (150 + 10 * k)), w, h).to_op())
    b_vr, b_vm = vr.stats("path_vr")[1], vr.stats("path_vm")[1]
    mixed, recs, rc = vr.process(srcs, ops)
    assert rc == 0 and all(r.status == 0 for r in recs)
    assert vr.stats("path_vm")[1] - b_vm == len(srcs) and vr.stats("path_vr")[1] == b_vr  # > 8 classes
    assert np.array_equal(mixed[0], alone[0])
    vr.close()


ROLE_CASES = [
    (1920, 1080, "w_500", 6),  # cfg2: 3 output blocks a strip (4 loaders need <= 2: stays at 2)
    (3840, 2160, "w_512,h_512,c_1", 2),
    (6000, 4000, "w_400,h_400,c_1,r_90,clsp_Gray", 2),
    (4000, 3000, "w_150", 2),  # uneven rows: the 8-row pair classes with 4 loaders
    (3000, 2000, "w_300,h_250,c_1", 3),
    (333, 517, "w_97", 4),
]


_VM_REF = {}


def _vm_ref(vm, W, H, opts, n):
    """k_rs_vm's outputs of a ROLE_CASES entry, computed once per module (the
    four role splits compare against the same bytes)"""
    key = (W, H, opts, n)
    if key not in _VM_REF:
        op = ImageProcessor(OptionsBag(opts), W, H).to_op()
        oa, _, rca = vm.process([synth_rgb(W, H, 900 + k) for k in range(n)], [op] * n)
        assert rca == 0
        _VM_REF[key] = oa
    return _VM_REF[key]


@pytest.mark.parametrize("nl,pbuf", [(2, 1), (2, 2), (4, 1), (4, 2)])
def test_vr_role_splits_and_plane_buffers(pair, nl, pbuf):
    """every loader-wave count (FI_VR_NL, where valid) and plane-buffer count
    (FI_VR_PBUF, where the ring fits) gives k_rs_vm's bytes"""
    _, vm = pair
    ctx = _context_with({"FI_VR_RS": "1", "FI_FORCE_GENERIC": "0", "FI_VR_NL": str(nl), "FI_VR_PBUF": str(pbuf)})
    try:
        for W, H, opts, n in ROLE_CASES:
            op = ImageProcessor(OptionsBag(opts), W, H).to_op()
            srcs = [synth_rgb(W, H, 900 + k) for k in range(n)]
            before = ctx.stats("path_vr")[1]
            ob, rb, rc = ctx.process(srcs, [op] * n)
            assert rc == 0 and all(r.status == 0 for r in rb), L.lib().fi_last_error()
            assert ctx.stats("path_vr")[1] == before + n
            oa = _vm_ref(vm, W, H, opts, n)
            for k in range(n):
                assert np.array_equal(ob[k], oa[k]), f"{opts} nl {nl} pbuf {pbuf} image {k}"
    finally:
        ctx.close()


def test_vr_split_launches(pair):
    """a batch that mixes one-block strips (4 loader waves) with wider ones in
    numbers that fill the chip twice runs as two k_rs_vr launches, the second
    on the forked stream beside the first; every image equals k_rs_vm's bytes"""
    vr, vm = pair
    geo = [(1920, 1080, "w_500"), (4000, 3000, "w_150"), (1920, 1080, "w_500"), (6000, 4000, "w_400,h_400,c_1,r_90,clsp_Gray")]
    uniq = sorted(set(geo))
    base = {g: [synth_rgb(g[0], g[1], 1300 + 7 * k + i) for i in range(2)] for k, g in enumerate(uniq)}
    srcs, ops, gk = [], [], []
    for k in range(80):
        g = geo[k % len(geo)]
        srcs.append(base[g][(k // len(geo)) % 2])
        ops.append(ImageProcessor(OptionsBag(g[2]), g[0], g[1]).to_op())
        gk.append((g, (k // len(geo)) % 2))
    before, forks = vr.stats("path_vr")[1], vr.stats("vr_fork")[1]
    ob, rb, rc = vr.process(srcs, ops)
    assert rc == 0 and all(r.status == 0 for r in rb), L.lib().fi_last_error()
    assert vr.stats("path_vr")[1] == before + len(srcs)
    assert vr.stats("vr_fork")[1] == forks + 1  # the second launch ran on the forked stream (FI_VR_FORK)
    for g in uniq:
        oa, _, rca = vm.process(base[g], [ImageProcessor(OptionsBag(g[2]), g[0], g[1]).to_op()] * 2)
        assert rca == 0
        for k in range(len(srcs)):
            if gk[k][0] == g:
                assert np.array_equal(ob[k], oa[gk[k][1]]), f"{g} image {k}: split k_rs_vr != k_rs_vm"


def test_narrow_strips_switch(pair):
    """FI_VR_NARROW=0 keeps 64-px strips (four 16-px blocks at 1/2) on k_rs_vm;
    the default builds them at 48 px for k_rs_vr; both give k_rs_vm's bytes of
    the default context's 64-px tables (the pixels do not depend on the strip
    width)."""
    vr, vm = pair
    W, H, opts = 640, 480, "w_320"
    op = ImageProcessor(OptionsBag(opts), W, H).to_op()
    srcs = [synth_rgb(W, H, 4100 + k) for k in range(3)]
    wide = _context_with({"FI_VR_RS": "1", "FI_FORCE_GENERIC": "0", "FI_VR_NARROW": "0"})
    try:
        b = wide.stats("path_vm")[1]
        ow, rw, rcw = wide.process(srcs, [op] * 3)
        assert rcw == 0 and wide.stats("path_vm")[1] == b + 3
        b = vr.stats("path_vr")[1]
        on, rn, rcn = vr.process(srcs, [op] * 3)
        assert rcn == 0 and vr.stats("path_vr")[1] == b + 3
        om, _, rcm = vm.process(srcs, [op] * 3)
        assert rcm == 0
        for k in range(3):
            assert np.array_equal(on[k], om[k]) and np.array_equal(ow[k], om[k])
    finally:
        wide.close()
