"""CPU: the progressive JPEG path's host side -- the multi-scan parser and the
scan scheduler (fi_jpeg_info_ex under FI_JPEG_PROGRESSIVE), and the four
jdphuff.c block procedures of fi_jpeg_prog.h run on the CPU
(fi_debug_jpeg_coefs_host), which are the ones k_jpeg_prog runs on the device.

The entropy core is checked exactly: for gray progressive files its
coefficients, dequantised and put through jidctint.c's islow IDCT (restated
here with numpy int32 and k_jpeg_idct's constants), must equal Pillow's
(libjpeg-turbo's) pixels.  The same code then runs under ASan/UBSan from a
stand-alone driver (tests/native/jpeg_prog_driver.cpp)."""
import io
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
from PIL import Image

from flyimg_amd import _lib as L
from flyimg_amd.runtime import jpeg_coefs_host, jpeg_info, jpeg_scan_info, jpeg_scan_status

from tests import _jpeg_files
from tests._jpeg_files import ZZ, _idct_plane, _islow_1d  # noqa: F401  (the integer-exact plane reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _photo(w, h, seed=3):
    """Smooth structure plus a little noise: every scan of the script carries data."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([128 + 100 * np.sin(x / 7.0 + c) * np.cos(y / 5.0 - c) for c in range(3)], -1)
    return np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def _jpeg(px, **kw):
    b = io.BytesIO()
    Image.fromarray(px).save(b, "JPEG", **kw)
    return b.getvalue()


def _golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _sos_list(blob):
    """(offset of the SOS marker, offset of its scan parameters Ss Se AhAl) of every scan."""
    out, p = [], 2
    while p + 4 <= len(blob):
        assert blob[p] == 0xFF
        m = blob[p + 1]
        if m == 0xD9:
            break
        ln = (blob[p + 2] << 8) | blob[p + 3]
        if m == 0xDA:
            out.append((p, p + 2 + ln - 3))
            q = p + 2 + ln
            while not (blob[q] == 0xFF and blob[q + 1] != 0 and not 0xD0 <= blob[q + 1] <= 0xD7):
                q += 1
            p = q
        else:
            p += 2 + ln
    return out


# ---- jpeg_scan_info known answers -------------------------------------------
SCAN_CASES = [("smart_crop.jpg", (1000, 750, 3, 7, 1)), ("extract-result.jpg", (200, 200, 3, 8, 2)),
              ("faces.jpg", (620, 349, 3, 9, 4))]


@pytest.mark.parametrize("name,want", SCAN_CASES, ids=[c[0] for c in SCAN_CASES])
def test_scan_info_golden_files(name, want):
    blob = _golden(name)
    assert jpeg_scan_info(blob) == want
    assert jpeg_info(blob, progressive=True) == want[:3]
    assert jpeg_info(blob) is None  # without the flag: host decode, as before


@pytest.mark.parametrize("ss", [0, 1, 2])
def test_scan_info_pillow_colour(ss):
    blob = _jpeg(_photo(97, 61), quality=90, subsampling=ss, progressive=True)
    assert jpeg_scan_info(blob) == (97, 61, 3, 10, 3)
    assert jpeg_info(blob) is None


def test_scan_info_pillow_gray_and_baseline():
    blob = _jpeg(_photo(97, 61)[..., 0], quality=90, progressive=True)
    assert jpeg_scan_info(blob) == (97, 61, 1, 6, 3)
    assert jpeg_info(blob) is None
    base = _jpeg(_photo(97, 61), quality=90)
    assert jpeg_scan_info(base) == (97, 61, 3, 1, 1)  # a baseline stream: one scan, one level
    assert jpeg_info(base) == jpeg_info(base, progressive=True) == (97, 61, 3)


# ---- rejections under the flag ----------------------------------------------
def _patched(blob, scan, ss=None, se=None, ahal=None):
    b = bytearray(blob)
    o = _sos_list(blob)[scan][1]
    if ss is not None:
        b[o] = ss
    if se is not None:
        b[o + 1] = se
    if ahal is not None:
        b[o + 2] = ahal
    return bytes(b)


def test_rejections_under_the_flag():
    blob = _jpeg(_photo(97, 61), quality=90, subsampling=2, progressive=True)
    sos = _sos_list(blob)
    # Pillow's (libjpeg's default) script: DC of all components, Y 1-5, Cr, Cb, Y 6-63, then the refinements
    params = [tuple(blob[o:o + 3]) for _, o in sos]
    assert params[0] == (0, 0, 0x01) and params[1] == (1, 5, 0x02) and params[5] == (1, 63, 0x21)
    assert jpeg_scan_status(blob)[0] == L.FI_OK
    # last scan removed, EOI appended: incomplete (libjpeg smooths such a file's blocks)
    assert jpeg_scan_status(blob[:sos[-1][0]] + b"\xff\xd9") == (L.FI_EUNSUPPORTED, None)
    assert jpeg_scan_info(blob[:sos[-1][0]] + b"\xff\xd9") is None
    # JERR_BAD_PROGRESSION
    assert jpeg_scan_status(_patched(blob, 1, ss=6))[0] == L.FI_EINVAL          # Ss > Se
    assert jpeg_scan_status(_patched(blob, 0, ss=0, se=5))[0] == L.FI_EINVAL    # Ss = 0, Se = 5
    assert jpeg_scan_status(_patched(blob, 1, se=64))[0] == L.FI_EINVAL         # Se > 63
    assert jpeg_scan_status(_patched(blob, 1, ahal=0x20))[0] == L.FI_EINVAL     # Al != Ah - 1
    assert jpeg_scan_status(_patched(blob, 1, ahal=0x0E))[0] == L.FI_EINVAL     # Al > 13
    # an AC scan with two components
    p = sos[1][0]
    ids = (blob[sos[0][0] + 5], blob[sos[0][0] + 7])
    two = blob[:p] + bytes([0xFF, 0xDA, 0, 10, 2, ids[0], 0x00, ids[1], 0x11, 1, 5, 0x02]) + blob[p + 10:]
    assert jpeg_scan_status(two)[0] == L.FI_EINVAL
    # a refinement whose Ah is not the Al sent before (valid for libjpeg, with a warning)
    assert jpeg_scan_status(_patched(blob, 5, ahal=0x32))[0] == L.FI_EUNSUPPORTED
    # data after EOI; EOI missing
    assert jpeg_scan_status(blob + b"\x00")[0] == L.FI_EUNSUPPORTED
    assert jpeg_scan_status(blob + b"\xff\xd9")[0] == L.FI_EUNSUPPORTED
    assert jpeg_scan_status(blob[:-2])[0] == L.FI_EUNSUPPORTED
    # cut off anywhere after the first scan's header, inside a scan or between two: truncated
    first = sos[0][1] + 3
    assert {jpeg_scan_status(blob[:n])[0] for n in range(first, len(blob))} == {L.FI_EUNSUPPORTED}
    # CMYK
    b = io.BytesIO()
    Image.fromarray(_photo(33, 17)).convert("CMYK").save(b, "JPEG", progressive=True)
    assert jpeg_scan_status(b.getvalue())[0] == L.FI_EUNSUPPORTED
    # and the host decoder turns the same streams down
    assert jpeg_coefs_host(blob[:-2]) is None and jpeg_coefs_host(_patched(blob, 1, ss=6)) is None
    assert jpeg_coefs_host(blob, progressive=False) is None


# ---- the host entropy core, exact -------------------------------------------
GRAY_CASES = [(1, 1, 30), (1, 1, 90), (33, 17, 30), (33, 17, 90), (97, 61, 30), (97, 61, 90)]


@pytest.mark.parametrize("w,h,q", GRAY_CASES, ids=[f"{w}x{h}q{q}" for w, h, q in GRAY_CASES])
def test_host_entropy_core_matches_pillow_gray(w, h, q):
    blob = _jpeg(_photo(w, h)[..., 0], quality=q, progressive=True)
    assert jpeg_scan_info(blob)[3] > 1
    coefs, qts = jpeg_coefs_host(blob)
    got = _idct_plane(coefs[0], qts[0])[:h, :w]
    want = np.asarray(Image.open(io.BytesIO(blob)))
    assert np.array_equal(got, want)


def test_host_entropy_core_long_eobrun_flat():
    """A flat 333x211 image at q30: 42 x 27 = 1134 blocks whose AC bands are
    one end-of-band run (EOBRUN carries over more than 1000 blocks)."""
    blob = _jpeg(np.full((211, 333), 77, np.uint8), quality=30, progressive=True)
    coefs, qts = jpeg_coefs_host(blob)
    assert coefs[0].shape == (27, 42, 64) and not coefs[0][..., 1:].any()
    got = _idct_plane(coefs[0], qts[0])[:211, :333]
    assert np.array_equal(got, np.asarray(Image.open(io.BytesIO(blob))))


def test_host_entropy_core_component_raster_of_subsampled_colour():
    """17x33 at 4:2:0: the luma raster of the AC scans is 3 x 5 blocks inside the
    4 x 6 padded MCU grid.  Luma needs no upsampling: IDCT of component 0 =
    Pillow's Y channel (draft-free YCbCr decode)."""
    blob = _jpeg(_photo(17, 33), quality=90, subsampling=2, progressive=True)
    coefs, qts = jpeg_coefs_host(blob)
    assert coefs[0].shape == (6, 4, 64) and coefs[1].shape == (3, 2, 64)
    assert not coefs[0][5, :, 1:].any() and not coefs[0][:, 3, 1:].any()  # outside the raster: DC only
    im = Image.open(io.BytesIO(blob))
    im.draft("YCbCr", im.size)
    y = np.asarray(im.convert("YCbCr") if im.mode != "YCbCr" else im)[..., 0]
    assert np.array_equal(_idct_plane(coefs[0], qts[0])[:33, :17], y)


# ---- sanitizers ---------------------------------------------------------------
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_progressive_host_path_under_asan_ubsan():
    """Parser, scheduler and host entropy core (the device kernel's block
    procedures) on the golden progressive files and Pillow-written ones: every
    7th truncation and 3000 seeded mutations each, exact-size buffers."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "jpeg_prog_driver")
        csrc = os.path.join(ROOT, "flyimg_amd", "csrc")
        subprocess.run([hipcc, "-std=c++17", "-fno-gpu-sanitize", *SAN, "-pthread", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests/native/jpeg_prog_driver.cpp"),
                        os.path.join(csrc, "fi_jpeg_parse.cpp"), os.path.join(csrc, "fi_jpeg_prog_host.cpp"),
                        "-o", exe], check=True, capture_output=True, timeout=300)
        files = [os.path.join(GOLDEN, n) for n, _ in SCAN_CASES]
        px = _photo(53, 37)
        made = {"p444.jpg": _jpeg(px, quality=90, subsampling=0, progressive=True),
                "p420r.jpg": _jpeg(px, quality=75, subsampling=2, progressive=True, restart_marker_blocks=2),
                "pgray.jpg": _jpeg(px[..., 0], quality=80, progressive=True)}
        for name, blob in made.items():
            files.append(os.path.join(d, name))
            with open(files[-1], "wb") as f:
                f.write(blob)
        # ... and damaged progressive streams of tests/_jpeg_files.py: scans and intervals cut short, restart
        # markers lost or renumbered (decoded, or handed to the host by the parser or the entropy core)
        files.append("--damaged")
        for dm in _jpeg_files.corpus_b():
            if dm.progressive and ("pgrey_scan" in dm.name or "pgrey_dri_scan_3" in dm.name or "p420_scan_5" in dm.name):
                files.append(os.path.join(d, dm.name + ".jpg"))
                with open(files[-1], "wb") as f:
                    f.write(dm.blob)
        r = subprocess.run([exe, *files], capture_output=True, text=True, timeout=600, env=ENV)
        assert r.returncode == 0, r.stderr[-4000:]
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        assert r.stdout.startswith("DONE ") and int(r.stdout.split()[1]) > len(files) * 3000
