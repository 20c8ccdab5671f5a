"""The adversarial contents of tests/_adversarial.py have teeth (oracle only,
no GPU): a numpy restatement of the oracle's two resample passes built from
its own tap hook (or_im_axis_taps) equals orc.im_convert bit for bit on every
case tests/test_gpu_adversarial.py runs, and the same restatement WITHOUT the
ClampToQuantum saturation between the passes -- a kernel that only clamps at
the end -- is off by more than 1 LSB on >= 5 % of the pixels of every checker
case.  Also here: the oracle keeps
flats flat, the GPU file's boundary-band assertion excludes < 30 % of a
case's pixels, and the smartcrop checkers saturate the oracle's prescale
(pil_clip8) at both ends."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import oracle as orc
from tests import _adversarial as A
from tests._planner import PLANNER_SRCS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_flags(case):
    f = orc.FLAG_THUMBNAIL if case.op in ("thumb", "enlarge") else 0
    f |= orc.FLAG_SHRINK if case.op in ("thumb", "resize") else 0
    f |= (orc.FLAG_FILL | orc.FLAG_EXTENT) if case.fill else 0
    f |= orc.FLAG_GRAY if case.gray else 0
    f |= orc.FLAG_ROTATE if case.rot else 0
    return f


def oracle_convert(case, src):
    return orc.im_convert(src, case.tw, case.th, oracle_flags(case), rotate=case.rot)


def resized_size(case):
    return orc.im_meta_geometry(case.W, case.H, case.tw, case.th, case.fill, case.op != "enlarge")


def _axis_taps(W, H, ow, oh, thumb, axis):
    """[(first source index, f64 weights)] per output index, from the oracle's hook"""
    L = orc.lib()
    L.or_im_axis_taps.argtypes = [ctypes.c_int] * 8 + [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double),
                                                        ctypes.c_int]
    buf = np.zeros(8192)
    out = []
    for o in range(oh if axis else ow):
        s = ctypes.c_int(-1)
        n = L.or_im_axis_taps(W, H, ow, oh, int(thumb), 0, axis, o, ctypes.byref(s),
                              buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), buf.size)
        assert n >= 0, (W, H, ow, oh, axis, o)
        out.append((s.value, buf[:n].copy()))
    return out


def _clamp_to_quantum(v, saturate=True):
    """ClampToQuantum; saturate=False keeps the rounding and drops the clamp"""
    r = np.floor(v + 0.5)
    if not saturate:
        return r
    return np.where(v <= 0.0, 0.0, np.where(v >= 65535.0, 65535.0, r))


def _pass(q, taps, axis):
    """one filter pass over axis (1 = rows / VerticalFilter), f64, summed tap by
    tap in the oracle's order"""
    q = q if axis else q.transpose(1, 0, 2)
    out = np.empty((len(taps),) + q.shape[1:])
    for o, (s, w) in enumerate(taps):
        acc = np.zeros(q.shape[1:])
        for i in range(len(w)):
            acc = acc + w[i] * q[s + i]
        out[o] = acc
    return out if axis else out.transpose(1, 0, 2)


def restate_q16(src, ow, oh, thumb, interpass_clamp=True):
    """ResizeImage of an 8-bit RGB image -> Q16 (as f64), IM's pass order
    (horizontal first when x_factor > y_factor, factors taken after the
    thumbnail sample pre-step)"""
    H, W = src.shape[:2]
    sample = bool(thumb) and bool(orc.lib().or_im_thumbnail_uses_sample(W, H, ow, oh))
    iw, ih = (5 * ow, 5 * oh) if sample else (W, H)
    hfirst = (ow / iw) > (oh / ih)
    tx, ty = _axis_taps(W, H, ow, oh, thumb, 0), _axis_taps(W, H, ow, oh, thumb, 1)
    q = src.astype(np.float64) * 257.0
    first, second = ((tx, 0), (ty, 1)) if hfirst else ((ty, 1), (tx, 0))
    mid = _clamp_to_quantum(_pass(q, *first), interpass_clamp)
    return _clamp_to_quantum(_pass(mid, *second)), hfirst


def restate(case, src, interpass_clamp=True):
    """the whole convert of a case: resize, -extent (Center), -colorspace Gray, -rotate"""
    ow, oh = resized_size(case)
    q, hfirst = restate_q16(src, ow, oh, case.op != "resize", interpass_clamp)
    assert hfirst == case.hfirst, case.name
    if case.fill:
        x0, y0 = orc.im_gravity_offset(ow, oh, case.tw, case.th)
        q = q[y0:y0 + case.th, x0:x0 + case.tw]
    if case.gray:
        q = _clamp_to_quantum(0.212656 * q[..., 0] + 0.715158 * q[..., 1] + 0.072186 * q[..., 2])
    out = A.q16_to_u8(q)
    return np.rot90(out, -(case.rot // 90)) if case.rot else out


@functools.lru_cache(maxsize=None)
def _restated(name, kind, clamp):
    case = RC[name]
    return restate(case, A.content(case, kind), clamp)


RC = {c.name: c for c in A.RESAMPLE_CASES}


@pytest.mark.parametrize("kind", A.CONTENTS)
@pytest.mark.parametrize("name", A.CASE_IDS)
def test_restatement_equals_oracle(name, kind):
    """numpy passes over or_im_axis_taps == orc.im_convert, bit for bit: pins
    the tap hook, the pass order and the clamp placement the mutant test edits"""
    case = RC[name]
    ref = oracle_convert(case, A.content(case, kind))
    got = _restated(name, kind, True)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref), int((got != ref).sum())


@pytest.mark.parametrize("name", A.CASE_IDS)
def test_interpass_clamp_mutant_is_visible_on_checkers(name):
    """without the saturation between the passes the result is off by > 1 LSB
    on >= 5 % of the pixels (16-31 % measured)"""
    case = RC[name]
    good, bad = _restated(name, "checker", True), _restated(name, "checker", False)
    off = float((np.abs(good.astype(np.int16) - bad.astype(np.int16)) > 1).mean())
    print(f"{name}: block {case.block}: {100 * off:.1f} % of pixels off by > 1")
    assert off >= 0.05, (name, off)


@pytest.mark.parametrize("name", A.CASE_IDS)
def test_oracle_keeps_flats_flat(name):
    case = RC[name]
    for v in A.FLAT_VALUES:
        ref = oracle_convert(case, A.flat(case.W, case.H, v))
        assert ref.size and (ref == v).all(), (name, v)


# --- boundary band -------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def vr_quant_bound_output():
    """stdout of tests/native/vr_quant_bound.cpp (None without hipcc)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    with tempfile.TemporaryDirectory() as d:
        exe, obj = os.path.join(d, "vqb"), os.path.join(d, "fi_oracle.o")
        subprocess.run(["gcc", "-O2", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-fno-fast-math", "-c",
                        os.path.join(ROOT, "oracle/fi_oracle.c"), "-o", obj], check=True, capture_output=True,
                       timeout=300)
        subprocess.run([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests/native/vr_quant_bound.cpp"),
                        *PLANNER_SRCS, "-Xlinker", obj, "-o", exe, "-lm"],
                       check=True, capture_output=True, timeout=300)
        r = subprocess.run([exe, "adversarial"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_band_e_is_the_proven_bound():
    """A.BAND_E (what the GPU file's band assertion moves the oracle's Q16 value
    by) is no smaller than the worst-case |k_rs_vr - oracle| in Q16 units that
    vr_quant_bound derives from each geometry's own tables, rounded up -- and
    no larger, so the band is as narrow as the proof allows"""
    out = vr_quant_bound_output()
    if out is None:
        pytest.skip("hipcc not available")
    for case in A.RESAMPLE_CASES:
        m = re.search(re.escape(case.name) + r": .*E ([0-9.]+) Q16", out)
        if case.cls != "vr":  # no k_rs_vr tables to bound: not a band case
            want = "horizontal first" if case.hfirst else "k_rs_vm's class"
            assert re.search(re.escape(case.name) + ": " + want, out) and case.band_block is None, case.name
            continue
        assert m, (case.name, out)
        if case.band_block is not None:
            assert A.BAND_E[case.name] == int(np.ceil(float(m.group(1)))), (case.name, m.group(1))
    assert sorted(A.BAND_E) == sorted(c.name for c in A.RESAMPLE_CASES if c.band_block is not None)


BAND = [(c.name, k) for c in A.RESAMPLE_CASES if c.band_block is not None for k in A.band_contents(c)]


@pytest.mark.parametrize("name,kind", BAND, ids=[f"{n}-{k}" for n, k in BAND])
def test_band_excludes_under_30_percent(name, kind):
    """the band assertion stays a per-pixel check: at most 30 % of a case's
    samples lie within E of a byte boundary (issue's cap)"""
    case = RC[name]
    ow, oh = resized_size(case)
    src = A.content(case, kind, band=True)
    q = orc.im_resize_q16(src, ow, oh, thumbnail=case.op != "resize")
    assert np.array_equal(A.q16_to_u8(q), oracle_convert(case, src))  # the Q16 image IS im_convert's
    share = 1.0 - float(A.band_mask(q, A.BAND_E[name]).mean())
    print(f"{name} {kind}: E {A.BAND_E[name]}: {100 * share:.1f} % excluded")
    assert share <= 0.30, (name, kind, share)


# --- smartcrop prescale saturation --------------------------------------------
@pytest.mark.parametrize("W,H,gray", A.SC_SIZES)
@pytest.mark.parametrize("kind", ["checker5", "checker9"])
def test_smartcrop_checkers_saturate_the_prescale(W, H, gray, kind):
    """>= 5 % of the oracle's prescaled bytes at 0 and >= 5 % at 255: pil_clip8
    clips both ways on these inputs"""
    pre = orc.sc_crop(A.sc_source(W, H, gray, kind), 100, 100)["prescaled"]
    lo, hi = float((pre == 0).mean()), float((pre == 255).mean())
    print(f"{W}x{H} {kind}: prescaled {pre.shape[1]}x{pre.shape[0]}: {100 * lo:.1f} % at 0, {100 * hi:.1f} % at 255")
    assert lo >= 0.05 and hi >= 0.05, (lo, hi)
