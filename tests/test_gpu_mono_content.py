"""The -monochrome kernels (fi_mono.hip: k_mono_stats, k_mono_dither) on the
crafted content of tests/_mono_content.py, bit for bit against the oracle's
or_im_monochrome at rotations 0, 90, 180 and 270 -- tests/test_mono_content_cpu.py
proved on the oracle and the literal that each input reaches its branch -- then
the hook with a destination stride wider than the row, and one pipeline call
with nine images whose geometry is the identity, so that several images go
through one launch and every byte still has to be the oracle's."""
import numpy as np
import pytest

from flyimg_amd import _lib as L
from flyimg_amd.runtime import Context, Op
from oracle import oracle as orc

from . import _mono_content as C

pytestmark = pytest.mark.gpu

CASES = C.kernel_cases()
_REF = {}


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _ref(name):
    if name not in _REF:
        _REF[name] = orc.im_monochrome(CASES[name])
        _REF[name].setflags(write=False)
    return _REF[name]


def _mismatches(ctx, g, ref):
    """the rotations at which the kernels' bytes are not the oracle's, with counts"""
    bad = []
    for rot in C.ROTS:
        want = np.rot90(ref, -rot // 90)
        got = ctx.monochrome_q16(g, rot)
        if got.shape != want.shape:
            bad.append(f"rot {rot}: shape {got.shape}")
        elif not np.array_equal(got, want):
            bad.append(f"rot {rot}: {(got != want).sum()} of {got.size} pixels")
    return bad


@pytest.mark.parametrize("name", list(CASES))
def test_crafted_input_every_rotation(ctx, name):
    bad = _mismatches(ctx, CASES[name], _ref(name))
    assert not bad, f"{name} {CASES[name].shape}: " + "; ".join(bad)


def test_histogram_sweep(ctx):
    """200 seeded histograms with the stretch owned; stops at the first failing seed"""
    for seed in range(C.SWEEP):
        kind, g, _ = C.sweep_image(seed)
        bad = _mismatches(ctx, g, orc.im_monochrome(g))
        assert not bad, f"seed {seed} ({kind}, {g.shape}): " + "; ".join(bad)


@pytest.mark.parametrize("name", C.WIDE_STRIDE)
def test_wide_destination_stride(ctx, name):
    """out_stride = ow + 13: the payload is the oracle's, and the 13 bytes behind
    every row are still the zeros the hook cleared the buffer to"""
    g = np.ascontiguousarray(CASES[name])
    h, w = g.shape
    for rot in C.ROTS:
        want = np.rot90(_ref(name), -rot // 90)
        oh, ow = want.shape
        out = np.full((oh, ow + 13), 0xA5, np.uint8)
        L.check(L.lib().fi_debug_monochrome(ctx.h, g.ctypes.data, w, h, rot, out.ctypes.data, ow + 13))
        assert np.array_equal(out[:, :ow], want), f"{name} rot {rot}: {(out[:, :ow] != want).sum()} pixels"
        assert not out[:, ow:].any(), f"{name} rot {rot}: {np.count_nonzero(out[:, ow:])} tail bytes written"


def _op(tw, th, window, rot, mono):
    f = L.FI_OP_THUMBNAIL | (L.FI_OP_MONOCHROME if mono else 0) | (L.FI_OP_ROTATE if rot else 0)
    if window:
        f |= L.FI_GEOM_FILL | L.FI_OP_EXTENT
    return Op(tw, th, f, L.GRAVITY["Center"], rot)


def test_pipeline_batch_of_monochrome_images(ctx):
    """Nine images in one process call, eight of them -monochrome (one launch
    of the two kernels with n = 8): every output is the oracle's convert and
    the bytes the image gives alone; the plain neighbour in the middle too."""
    batch = C.pipeline_batch()
    srcs = [b[1] for b in batch]
    ops = [_op(*b[2:]) for b in batch]
    outs, recs, rc = ctx.process(srcs, ops)
    assert rc == 0 and all(r.status == 0 for r in recs), ([r.status for r in recs], L.lib().fi_last_error())
    bad = []
    for (name, src, tw, th, window, rot, mono), op, out in zip(batch, ops, outs):
        solo, srec, src_rc = ctx.process([src], [op])
        assert src_rc == 0 and srec[0].status == 0, (name, L.lib().fi_last_error())
        if out.shape != solo[0].shape or not np.array_equal(out, solo[0]):
            bad.append(f"{name}: not its solo run's bytes")
        if mono:
            ref = C.pipeline_reference(src, tw, th, window, rot, True)
            if out.shape != ref.shape:
                bad.append(f"{name}: shape {out.shape}, oracle {ref.shape}")
            elif not np.array_equal(out, ref):
                bad.append(f"{name}: {(out != ref).sum()} of {ref.size} pixels off the oracle")
    assert not bad, "; ".join(bad)
