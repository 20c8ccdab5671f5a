"""Host model of the progressive GPU JPEG encoder (fi_jpeg_pwrite.cpp with
fi_jpeg_pcore.h, the code the kernels compile too), no GPU: Pillow's
progressive restart-row file -> its quantised coefficients
(fi_debug_jpeg_coefs_host) -> fi_debug_jpeg_prog_write_host must give the
file back byte for byte -- scan script, block procedures, EOB runs, correction
bits, per-scan optimal tables, DHT / DRI / SOS layout.  One image makes the
correction-bit buffer end EOB runs early; the size bound covers noise at
quality 100; the writer runs stand-alone under ASan/UBSan
(tests/native/jpeg_pwrite_driver.cpp, its own process, nothing preloaded)."""
import io
import os
import subprocess
import tempfile

import numpy as np
import pytest
from PIL import Image, ImageFile

from flyimg_amd import _lib as L
from flyimg_amd.runtime import jpeg_coefs_host, jpeg_encode_bound, jpeg_prog_write_host
from flyimg_amd.synth import synth_rgb

from . import _encoder_content as E
from .test_jpeg_encode_cpu import GEOMETRIES
from .test_sanitize_cpu import ENV, ROOT, SAN, _compiler

SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 23), (40, 56), (33, 65), (333, 211), (500, 281)]
QUALITIES = [1, 30, 50, 89, 90, 100]
# The flush image: gray 256x16, tiled from the binary 8x8 block of
# default_rng(FLUSH_SEED) (first seed of a search from 0 whose quantised AC
# coefficients at quality 100 include no +-1): every block row of the last scan
# is one EOB run that gathers 63 correction bits per block.
FLUSH_SEED = 0


def pillow_progressive(px, quality, subsampling=0):
    """libjpeg-turbo's progressive file with one restart interval per block row."""
    b = io.BytesIO()
    kw = dict(subsampling=subsampling) if px.ndim == 3 else {}
    # (Pillow sizes libjpeg's output buffer from the pixel count, which noise at quality 100 exceeds)
    old, ImageFile.MAXBLOCK = ImageFile.MAXBLOCK, max(ImageFile.MAXBLOCK, 1 << 24)
    try:
        Image.fromarray(px).save(b, "JPEG", quality=quality, progressive=True, restart_marker_rows=1, **kw)
    finally:
        ImageFile.MAXBLOCK = old
    return b.getvalue()


def same(got, ref, what):
    assert got is not None, what
    if got != ref:
        k = next((i for i in range(min(len(got), len(ref))) if got[i] != ref[i]), min(len(got), len(ref)))
        raise AssertionError(f"{what}: {len(got)} bytes against Pillow's {len(ref)}, first difference at byte {k}")


def flush_image():
    blk = (np.random.default_rng(FLUSH_SEED).integers(0, 2, (8, 8)) * 255).astype(np.uint8)
    return np.tile(blk, (2, 32))


def _round_trip(px, quality, subsampling, what):
    ref = pillow_progressive(px, quality, subsampling)
    co, _ = jpeg_coefs_host(ref)
    h, w = px.shape[:2]
    got, flushes = jpeg_prog_write_host(co, w, h, 3 if px.ndim == 3 else 1, quality, subsampling)
    same(got, ref, what)
    assert len(got) <= jpeg_encode_bound(w, h, 3 if px.ndim == 3 else 1, quality, subsampling, progressive=True)
    return flushes


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_model_round_trip_sizes(w, h):
    px = synth_rgb(w, h, 11 + w + h)
    _round_trip(px, 90, 0, f"{w}x{h} 4:4:4 q90")
    _round_trip(px, 75, 2, f"{w}x{h} 4:2:0 q75")
    _round_trip(np.ascontiguousarray(px[..., 1]), 80, 0, f"{w}x{h} gray q80")


@pytest.mark.parametrize("q", QUALITIES)
def test_model_round_trip_qualities(q):
    px = synth_rgb(97, 61, 5)
    _round_trip(px, q, 0, f"q{q} 4:4:4")
    _round_trip(px, q, 2, f"q{q} 4:2:0")


@pytest.mark.parametrize("ss", [0, 2])
def test_model_round_trip_noise(ss):
    px = np.random.default_rng(ss).integers(0, 256, (157, 211, 3), dtype=np.uint8)
    _round_trip(px, 100, ss, f"noise ss{ss}")


def test_model_flushes_the_correction_buffer_inside_an_eob_run():
    px = flush_image()
    co, _ = jpeg_coefs_host(pillow_progressive(px, 100))
    ac = np.abs(co[0][..., 1:].astype(np.int32))
    assert not (ac == 1).any() and (ac > 1).all()  # the last scan: no newly nonzero coefficient, 63 correction bits
    assert _round_trip(px, 100, 0, "flush image") >= 1


@pytest.mark.parametrize("mode", ["444", "420", "gray"])
def test_progressive_bound_covers_noise_at_q100(mode):
    rng = np.random.default_rng(7)
    for w, h in GEOMETRIES:
        px = rng.integers(0, 256, (h, w) if mode == "gray" else (h, w, 3), dtype=np.uint8)
        ss = 2 if mode == "420" else 0
        size = len(pillow_progressive(px, 100, ss))
        bound = jpeg_encode_bound(w, h, 1 if mode == "gray" else 3, 100, ss, progressive=True)
        assert size <= bound, (w, h, mode, size, bound)


def test_progressive_bound_rejects_bad_arguments():
    n = L.ctypes.c_size_t()
    f = L.lib().fi_jpeg_encode_bound_ex
    ref = L.ctypes.byref(n)
    P = L.FI_JPEG_ENC_PROGRESSIVE
    assert f(10, 10, 3, 90, 0, P, ref) == L.FI_OK and n.value > 0
    assert f(10, 10, 1, 90, 7, P, ref) == L.FI_OK  # subsampling is ignored for gray
    for c in (2, 4):
        assert f(10, 10, c, 90, 0, P, ref) == L.FI_EUNSUPPORTED
    assert f(10, 10, 3, 90, 1, P, ref) == L.FI_EUNSUPPORTED
    for q in (0, 101, -5):
        assert f(10, 10, 3, q, 0, P, ref) == L.FI_EINVAL
    for w, h in ((0, 10), (10, 0), (65536, 10), (10, 65536), (-1, 10)):
        assert f(w, h, 3, 90, 0, P, ref) == L.FI_EINVAL
    assert f(65535, 65535, 3, 100, 0, P, ref) == L.FI_OK
    assert f(10, 10, 3, 90, 0, P, None) == L.FI_EINVAL
    assert f(10, 10, 3, 90, 0, 2, ref) == L.FI_EINVAL  # an unknown flag
    # flags 0: the baseline bound
    assert f(97, 61, 3, 75, 2, 0, ref) == L.FI_OK and n.value == jpeg_encode_bound(97, 61, 3, 75, 2)


def test_model_rejects_coefficients_that_do_not_fit():
    co = np.zeros(64 * 3, np.int16)
    n, fl = L.ctypes.c_size_t(), L.ctypes.c_int32()
    out = np.empty(4096, np.uint8)
    f = L.lib().fi_debug_jpeg_prog_write_host
    args = (out.ctypes.data, out.size, L.ctypes.byref(n), L.ctypes.byref(fl))
    assert f(co.ctypes.data, co.size, 8, 8, 3, 90, 0, *args) == L.FI_OK and 0 < n.value <= out.size
    assert f(co.ctypes.data, co.size - 64, 8, 8, 3, 90, 0, *args) == L.FI_EINVAL
    assert f(co.ctypes.data, co.size, 8, 8, 3, 90, 2, *args) == L.FI_EINVAL  # 4:2:0 holds 6 blocks
    assert f(co.ctypes.data, co.size, 8, 8, 4, 90, 0, *args) == L.FI_EUNSUPPORTED
    assert f(co.ctypes.data, co.size, 8, 8, 3, 90, 0, out.ctypes.data, 10, L.ctypes.byref(n),
             L.ctypes.byref(fl)) == L.FI_ENOMEM and n.value > 10


def test_writer_under_asan_ubsan_matches_pillow():
    hipcc = _compiler("hipcc")
    cases = []
    for w, h in ((1, 1), (7, 9), (17, 23), (33, 65), (130, 129)):
        px = synth_rgb(w, h, 3 + w)
        cases += [(px, 90, 0), (px, 75, 2), (np.ascontiguousarray(px[..., 1]), 80, 0)]
    noise = np.random.default_rng(3).integers(0, 256, (45, 77, 3), dtype=np.uint8)
    cases += [(noise, 100, 0), (noise, 100, 2), (synth_rgb(97, 61, 5), 1, 2)]
    # crafted coefficients (tests/_encoder_content.py): the code-length limit, the refinement scan's
    # ZRL rules, the largest DC and AC categories, EOB runs of 4094 and 8188
    crafted = E.crafted()
    cases += [(c.px, c.quality, c.subsampling) for c in (
        crafted[n] for n in ("deep17_gray", "zero_runs_gray", "zero_runs_444", "dc_swing_gray", "dc_swing_444",
                             "dc_swing_420", "ac_max_gray", "ac_max_444", "long_eob_single"))]
    cases += [(flush_image(), 100, 0)]  # (stays the last one)
    bad = [(10, 10, 4, 90, 0), (10, 10, 3, 0, 0), (0, 5, 1, 50, 0), (10, 10, 3, 90, 1), (16, 16, 3, 90, 0)]
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "jpeg_pwrite")
        subprocess.run([hipcc, "-std=c++17", "-fno-gpu-sanitize", *SAN, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests/native/jpeg_pwrite_driver.cpp"),
                        os.path.join(ROOT, "flyimg_amd/csrc/fi_jpeg_pwrite.cpp"),
                        os.path.join(ROOT, "flyimg_amd/csrc/fi_jpeg_write.cpp"), "-o", exe],
                       check=True, capture_output=True, timeout=300)
        lines_in, refs = [], []
        for k, (px, q, s) in enumerate(cases):
            ref = pillow_progressive(px, q, s)
            co, _ = jpeg_coefs_host(ref)
            np.concatenate([c.ravel() for c in co]).astype("<i2").tofile(os.path.join(d, f"{k}.coef"))
            refs.append(ref)
            lines_in.append((px.shape[1], px.shape[0], 3 if px.ndim == 3 else 1, q, s))
        # (the last bad case has good settings and no coefficient file)
        stdin = "".join(" ".join(map(str, c)) + "\n" for c in lines_in + bad)
        r = subprocess.run([exe, d], input=stdin, capture_output=True, text=True, timeout=300, env=ENV)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        lines = r.stdout.split("\n")
        assert f"DONE {len(cases) + len(bad)}" in lines
        for k in range(len(bad)):
            assert "REJECT" in lines[len(cases) + k], lines[len(cases) + k]
        for k, (w, h, c, q, s) in enumerate(lines_in):
            same(open(os.path.join(d, f"{k}.jpg"), "rb").read(), refs[k], f"case {k}: {w}x{h}x{c} q{q} ss{s}")
            f = lines[k].split()
            assert int(f[2]) == len(refs[k]) and int(f[6]) == jpeg_encode_bound(w, h, c, q, s, progressive=True)
        assert int(lines[len(cases) - 1].split()[4]) >= 1  # the flush image's flushes
