"""Host side of the GPU decoder's views, no GPU: fi_jpeg_orientation against
the orientation Pillow's getexif yields (the one the host decode path
applies), codec.gpu_decodable's ``orient`` switch, and -- built stand-alone
under ASan/UBSan (tests/native/jpeg_view_driver.cpp, its own process, nothing
preloaded) -- the index map of fi_jpeg_view.h against Image.transpose and the
orientation reader over truncations and mutations of the hand-built headers."""
import ctypes
import io
import os
import subprocess
import tempfile

import numpy as np
import pytest
from PIL import Image

from flyimg_amd import _lib as L
from flyimg_amd.codec import gpu_decodable
from flyimg_amd.runtime import jpeg_orientation

from . import _orient_files as F
from .test_sanitize_cpu import ENV, ROOT, SAN, _compiler

PX = F.photo(40, 24)
BASE = F.jpeg(PX)


def _cases():
    """name -> (blob, must be determined)"""
    c = {}
    for k in range(10):
        c[f"pillow_{k}"] = (F.pillow_oriented(PX, k), True)
    for k in (1, 3, 6, 8):
        c[f"le_short_{k}"] = (F.splice(BASE, F.exif_app1(k, le=True)), True)
        c[f"be_short_{k}"] = (F.splice(BASE, F.exif_app1(k, le=False)), True)
    c["le_short_0"] = (F.splice(BASE, F.exif_app1(0)), True)
    c["be_short_9"] = (F.splice(BASE, F.exif_app1(9, le=False)), True)
    c["be_short_774"] = (F.splice(BASE, F.exif_app1(0x0306, le=False)), True)
    c["ifd_at_12"] = (F.splice(BASE, F.exif_app1(5, ifd_off=12)), True)
    c["no_orientation_tag"] = (F.splice(BASE, F.exif_app1(entries=[(0x0100, 4, 1, b"\x10\x00\x00\x00")])), True)
    c["exif_before_jfif"] = (F.splice(BASE, F.exif_app1(6), before_jfif=True), True)
    c["exif_after_jfif"] = (F.splice(BASE, F.exif_app1(8, le=False)), True)
    c["no_app1"] = (BASE, True)
    c["progressive_7"] = (F.splice(F.jpeg(PX, progressive=True), F.exif_app1(7)), True)
    c["xmp_beside_exif"] = (F.splice(BASE, F.exif_app1(3) + F.xmp_app1(6)), True)
    # the host decides (or agrees)
    c["long"] = (F.splice(BASE, F.exif_app1(6, typ=4)), False)
    c["long_be"] = (F.splice(BASE, F.exif_app1(6, typ=4, le=False)), False)
    c["count_2"] = (F.splice(BASE, F.exif_app1(6, count=2)), False)
    t = F.tiff(6)
    c["ifd_beyond"] = (F.splice(BASE, F.segment(0xE1, b"Exif\x00\x00" + t[:4] + b"\xa0\x0f\x00\x00" + t[8:])), False)
    c["truncated_table"] = (F.splice(BASE, F.segment(0xE1, b"Exif\x00\x00" + t[:8 + 2 + 12 + 5])), False)
    c["truncated_header"] = (F.splice(BASE, F.segment(0xE1, b"Exif\x00\x00" + t[:6])), False)
    c["two_exif"] = (F.splice(BASE, F.exif_app1(6) + F.exif_app1(8)), False)
    c["xmp_only"] = (F.splice(BASE, F.xmp_app1(6)), False)
    c["xmp_and_exif_without_tag"] = (
        F.splice(BASE, F.exif_app1(entries=[(0x0100, 4, 1, b"\x10\x00\x00\x00")]) + F.xmp_app1(8)), False)
    c["tag_twice"] = (F.splice(BASE, F.exif_app1(entries=[(0x0112, 3, 1, b"\x06\x00\x00\x00"),
                                                          (0x0112, 3, 1, b"\x08\x00\x00\x00")])), False)
    c["bigtiff_magic"] = (F.splice(BASE, F.segment(0xE1, b"Exif\x00\x00II+\x00" + F.tiff(6)[4:])), False)
    c["segment_past_data"] = (BASE[:2] + b"\xff\xe1\xff\xf0Exif\x00\x00" + F.tiff(6), False)
    return c


CASES = _cases()


def _pillow_orientation(blob):
    try:
        return F.host_orientation(blob)
    except Exception:  # noqa: BLE001 - the host path fails on it: any "cannot tell" is right
        return None


@pytest.mark.parametrize("name", list(CASES))
def test_orientation_is_pillows_or_undetermined(name):
    blob, determined = CASES[name]
    got = jpeg_orientation(blob)
    want = _pillow_orientation(blob)
    print(name, "library", got, "pillow", want)
    assert got is None or got == want, (name, got, want)
    if determined:
        assert got is not None and got == want, (name, got, want)


def test_orientation_expected_values():
    """The parity test's reference is Pillow; these pin what it must have said."""
    for k in range(10):
        assert jpeg_orientation(CASES[f"pillow_{k}"][0]) == (k if 2 <= k <= 8 else 1)
    assert jpeg_orientation(CASES["be_short_6"][0]) == 6
    assert jpeg_orientation(CASES["exif_before_jfif"][0]) == 6
    assert jpeg_orientation(CASES["progressive_7"][0]) == 7
    assert jpeg_orientation(CASES["xmp_beside_exif"][0]) == 3
    assert _pillow_orientation(CASES["xmp_only"][0]) == 6  # Pillow falls back to the XMP packet ...
    assert jpeg_orientation(CASES["xmp_only"][0]) is None  # ... which the library leaves to the host
    for name in ("two_exif", "long", "count_2", "ifd_beyond", "truncated_table", "segment_past_data"):
        assert jpeg_orientation(CASES[name][0]) is None, name


def test_orientation_status_codes():
    buf = io.BytesIO()
    Image.fromarray(PX).save(buf, "PNG")
    png = buf.getvalue()
    assert jpeg_orientation(png) is None and jpeg_orientation(b"") is None
    o = ctypes.c_int32(77)
    lib = L.lib()
    assert lib.fi_jpeg_orientation(png, len(png), ctypes.byref(o)) == L.FI_EINVAL
    xmp = CASES["xmp_only"][0]
    assert lib.fi_jpeg_orientation(xmp, len(xmp), ctypes.byref(o)) == L.FI_EUNSUPPORTED
    assert lib.fi_jpeg_orientation(BASE, 2, ctypes.byref(o)) == L.FI_EUNSUPPORTED  # SOI alone: no SOS
    assert o.value == 77  # untouched unless FI_OK
    assert lib.fi_jpeg_orientation(BASE, len(BASE), ctypes.byref(o)) == L.FI_OK and o.value == 1


def test_gpu_decodable_defaults_unchanged_and_orient_switch():
    px = F.photo(40, 24)
    rot = F.pillow_oriented(px, 6)
    assert gpu_decodable(rot) is None
    assert gpu_decodable(rot, False) is None
    assert gpu_decodable(rot, orient=True) == (24, 40, 3)
    assert gpu_decodable(F.pillow_oriented(px, 3), orient=True) == (40, 24, 3)
    assert gpu_decodable(BASE) == (40, 24, 3) == gpu_decodable(BASE, orient=True)
    assert gpu_decodable(F.pillow_oriented(F.photo(9, 31, gray=True), 5), orient=True) == (31, 9, 1)
    assert gpu_decodable(CASES["xmp_only"][0], orient=True) is None
    assert gpu_decodable(CASES["xmp_only"][0]) is None  # (Pillow reads the XMP orientation)
    prog = CASES["progressive_7"][0]
    assert gpu_decodable(prog, orient=True) is None
    assert gpu_decodable(prog, progressive=True, orient=True) == (24, 40, 3)


def test_abi_view_struct_and_symbols():
    assert ctypes.sizeof(L.FiJpegView) == 20
    assert [n for n, _ in L.FiJpegView._fields_] == ["orientation", "x", "y", "w", "h"]
    names = L.header_functions()
    assert "fi_jpeg_orientation" in names and "fi_jpeg_decode_device_view" in names
    lib = L.lib()
    assert hasattr(lib, "fi_jpeg_orientation") and hasattr(lib, "fi_jpeg_decode_device_view")
    assert lib.fi_abi_version() == 2


TRANSPOSE = {2: Image.Transpose.FLIP_LEFT_RIGHT, 3: Image.Transpose.ROTATE_180, 4: Image.Transpose.FLIP_TOP_BOTTOM,
             5: Image.Transpose.TRANSPOSE, 6: Image.Transpose.ROTATE_270, 7: Image.Transpose.TRANSVERSE,
             8: Image.Transpose.ROTATE_90}


@pytest.fixture(scope="module")
def driver():
    hipcc = _compiler("hipcc")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "jpeg_view_driver")
        subprocess.run([hipcc, "-std=c++17", "-fno-gpu-sanitize", *SAN, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests/native/jpeg_view_driver.cpp"),
                        os.path.join(ROOT, "flyimg_amd/csrc/fi_jpeg_parse.cpp"), "-o", exe],
                       check=True, capture_output=True, timeout=300)
        yield exe, d


def _clean(r):
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_index_map_matches_pillow_transpose(driver):
    exe, _ = driver
    r = subprocess.run([exe, "map"], capture_output=True, text=True, timeout=120, env=ENV)
    _clean(r)
    seen = set()
    for line in r.stdout.splitlines():
        head, pts = line.split(":")
        _, o, W, H = head.split()
        o, W, H = int(o), int(W), int(H)
        index = Image.fromarray(np.arange(W * H, dtype=np.uint8).reshape(H, W))  # pixel = sy * W + sx
        want = np.asarray(index.transpose(TRANSPOSE[o]) if o > 1 else index)
        got = [int(p.split(",")[1]) * W + int(p.split(",")[0]) for p in pts.split()]
        assert want.shape == ((W, H) if o >= 5 else (H, W))
        assert got == want.ravel().tolist(), (o, W, H)
        seen.add((o, W, H))
    assert seen == {(o, W, H) for o in range(1, 9) for W, H in ((5, 3), (1, 4))}


def test_orientation_reader_under_asan_ubsan(driver):
    """Every truncation and 2000 seeded single-byte mutations of the APP1
    bodies of each hand-built file; the stand-alone build agrees with the library."""
    exe, d = driver
    names = [n for n in CASES if not n.startswith("pillow_")]
    files = []
    for n in names:
        files.append(os.path.join(d, n + ".jpg"))
        with open(files[-1], "wb") as f:
            f.write(CASES[n][0])
    r = subprocess.run([exe, "fuzz", *files], capture_output=True, text=True, timeout=300, env=ENV)
    _clean(r)
    lines = r.stdout.splitlines()
    assert lines[-1].startswith("DONE") and int(lines[-1].split()[1]) > len(names) * 1000
    for line in lines[:-1]:
        _, i, rc, o = line.split()
        got = jpeg_orientation(CASES[names[int(i)]][0])
        assert (int(o) if int(rc) == 0 else None) == got, (names[int(i)], line)
