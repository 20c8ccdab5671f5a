"""Host side of the GPU JPEG encoder (fi_jpeg_write.cpp), no GPU: the size
bound fi_jpeg_encode_bound against Pillow's files of noise at quality 100, and
the header writer -- built stand-alone under ASan/UBSan
(tests/native/jpeg_write_driver.cpp, its own process, nothing preloaded) --
against the bytes of Pillow's file up to and including the SOS segment."""
import io
import os
import subprocess
import tempfile

import numpy as np
import pytest
from PIL import Image

from flyimg_amd import _lib as L
from flyimg_amd.runtime import jpeg_encode_bound

from .test_sanitize_cpu import ENV, ROOT, SAN, _compiler

GEOMETRIES = [(1, 1), (7, 9), (8, 8), (9, 9), (15, 17), (16, 16), (17, 23), (24, 40), (33, 65), (40, 56), (64, 100),
              (97, 61), (100, 3), (3, 100), (127, 129), (200, 8), (8, 200), (211, 157), (256, 256), (333, 211)]


def _pillow(px, quality, subsampling):
    b = io.BytesIO()
    kw = dict(subsampling=subsampling) if px.ndim == 3 else {}
    Image.fromarray(px).save(b, "JPEG", quality=quality, restart_marker_rows=1, **kw)
    return b.getvalue()


def _through_sos(blob):
    """The file's bytes up to and including the SOS segment."""
    i = 2
    while True:
        assert blob[i] == 0xFF
        seg = 2 + (blob[i + 2] << 8 | blob[i + 3])
        if blob[i + 1] == 0xDA:
            return blob[:i + seg]
        i += seg


@pytest.mark.parametrize("mode", ["444", "420", "gray"])
def test_encode_bound_covers_noise_at_q100(mode):
    rng = np.random.default_rng(7)
    for w, h in GEOMETRIES:
        px = rng.integers(0, 256, (h, w) if mode == "gray" else (h, w, 3), dtype=np.uint8)
        ss = 2 if mode == "420" else 0
        size = len(_pillow(px, 100, ss))
        bound = jpeg_encode_bound(w, h, 1 if mode == "gray" else 3, 100, ss)
        assert size <= bound, (w, h, mode, size, bound)


def test_encode_bound_rejects_bad_arguments():
    n = L.ctypes.c_size_t()
    f = L.lib().fi_jpeg_encode_bound
    ref = L.ctypes.byref(n)
    assert f(10, 10, 3, 90, 0, ref) == L.FI_OK and n.value > 0
    assert f(10, 10, 1, 90, 7, ref) == L.FI_OK  # subsampling is ignored for gray
    for c in (2, 4):
        assert f(10, 10, c, 90, 0, ref) == L.FI_EUNSUPPORTED
    assert f(10, 10, 3, 90, 1, ref) == L.FI_EUNSUPPORTED
    for q in (0, 101, -5):
        assert f(10, 10, 3, q, 0, ref) == L.FI_EINVAL
    for w, h in ((0, 10), (10, 0), (65536, 10), (10, 65536), (-1, 10)):
        assert f(w, h, 3, 90, 0, ref) == L.FI_EINVAL
    assert f(65535, 65535, 3, 100, 0, ref) == L.FI_OK
    assert f(10, 10, 3, 90, 0, None) == L.FI_EINVAL


def _header_cases():
    cases = []
    for w, h in ((1, 1), (7, 9), (8, 8), (16, 16), (17, 23), (40, 56), (33, 65), (333, 211), (500, 281)):
        cases += [(w, h, 3, 90, 0), (w, h, 3, 75, 2), (w, h, 1, 80, 0)]
    for q in (1, 30, 50, 89, 90, 100):
        cases += [(97, 61, 3, q, 0), (97, 61, 3, q, 2)]
    cases += [(65535, 65535, 3, 100, 2), (65535, 1, 1, 1, 0)]
    return cases


def test_header_writer_under_asan_ubsan_matches_pillow():
    hipcc = _compiler("hipcc")
    cases = _header_cases()
    bad = [(10, 10, 4, 90, 0), (10, 10, 3, 0, 0), (0, 5, 1, 50, 0), (10, 10, 3, 90, 1), (70000, 5, 3, 50, 2)]
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "jpeg_write")
        subprocess.run([hipcc, "-std=c++17", "-fno-gpu-sanitize", *SAN, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests/native/jpeg_write_driver.cpp"),
                        os.path.join(ROOT, "flyimg_amd/csrc/fi_jpeg_write.cpp"), "-o", exe],
                       check=True, capture_output=True, timeout=300)
        stdin = "".join(" ".join(map(str, c)) + "\n" for c in cases + bad)
        r = subprocess.run([exe, d], input=stdin, capture_output=True, text=True, timeout=300, env=ENV)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        lines = r.stdout.split("\n")
        assert f"DONE {len(cases) + len(bad)}" in lines
        for k in range(len(bad)):
            assert "REJECT" in lines[len(cases) + k], lines[len(cases) + k]
        for k, (w, h, c, q, s) in enumerate(cases):
            got = open(os.path.join(d, f"{k}.hdr"), "rb").read()
            if max(w, h) > 1000:  # too large to encode here: the frame header's fields only
                assert got[:2] == b"\xff\xd8" and bytes([h >> 8, h & 255, w >> 8, w & 255]) in got
                continue
            px = np.zeros((h, w, 3) if c == 3 else (h, w), np.uint8)
            assert got == _through_sos(_pillow(px, q, s)), (w, h, c, q, s)
            assert int(lines[k].split()[2]) == jpeg_encode_bound(w, h, c, q, s)
