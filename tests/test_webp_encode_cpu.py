"""Host side of the GPU lossless WebP encoder, no GPU: the size bound
fi_webp_encode_bound and the host form fi_debug_webp_encode_host -- the inline
code of fi_webp_enc.h the device runs, so its file is the device's file --
from the library and, built stand-alone under ASan/UBSan
(tests/native/webp_write_driver.cpp, its own process, nothing preloaded), from
the driver.  Lossless makes the check exact: Pillow (libwebp) and the literal
reader of tests/webp_literal.py must both return the input pixels."""
import io
import os
import subprocess
import tempfile

import numpy as np
import pytest
from PIL import Image

from flyimg_amd import _lib as L
from flyimg_amd.runtime import webp_encode_bound, webp_encode_host_form
from flyimg_amd.synth import synth_rgb

from . import webp_literal
from .test_sanitize_cpu import ENV, ROOT, SAN, _compiler

BOUND_GEOMETRIES = [(1, 1), (1, 7), (7, 1), (3, 5), (16, 17), (17, 16), (90, 91), (91, 91), (200, 200), (333, 211),
                    (16384, 1), (1, 16384)]
GEOMETRIES = [g for g in BOUND_GEOMETRIES if max(g) <= 333]
CONTENTS = ["synth", "flat", "checker", "noise", "tiled", "gradient"]


def channels(rgba, c):
    """RGBA -> the c-channel source: gray is the green plane."""
    return np.ascontiguousarray({1: rgba[:, :, 1:2], 2: rgba[:, :, [1, 3]], 3: rgba[:, :, :3], 4: rgba}[c])


def content(name, w, h, seed=0):
    """An RGBA image of the named content."""
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "synth":
        rgb = synth_rgb(w, h, 0x5EED + w + seed)
        return np.dstack([rgb, rgb[:, :, :1] ^ 0x55])
    if name == "flat":
        return np.broadcast_to(np.array([200, 10, 77, 128], np.uint8), (h, w, 4)).copy()
    if name == "checker":
        return np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[:, :, None], 4, 2)
    if name == "noise":
        return np.random.default_rng(w * 1000 + h + seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    if name == "tiled":
        tile = np.random.default_rng(45).integers(0, 256, (5, 4, 4), dtype=np.uint8)
        return np.tile(tile, (-(-h // 5), -(-w // 4), 1))[:h, :w].copy()
    if name == "gradient":
        # Two axes: every channel is a function of m = max(horizontal ramp, vertical ramp), so above the
        # diagonal the image depends on x alone (T predicts it exactly, L does not) and below it on y alone
        # (L predicts exactly, T does not): blocks on either side must choose different modes.  Alpha ramps
        # from 0 over a quarter of the image, whose colour must survive.
        m = np.maximum(xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1))
        return np.dstack([m, 255 - m, m // 2 + 17, np.clip(2 * m - 255, 0, 255)]).astype(np.uint8)
    raise KeyError(name)


def expected(px):
    """What a decoder returns for a c-channel source: (pixels, Pillow mode)."""
    c = px.shape[2]
    if c == 1:
        return np.repeat(px, 3, 2), "RGB"
    if c == 2:
        return np.dstack([px[:, :, :1]] * 3 + [px[:, :, 1:]]), "RGBA"
    return px, "RGB" if c == 3 else "RGBA"


def check_file(blob, px, literal=True):
    """Pillow and the literal reader return the source; -> the reader's result."""
    want, mode = expected(px)
    assert blob[:4] == b"RIFF" and blob[8:16] == b"WEBPVP8L" and len(blob) % 2 == 0
    im = Image.open(io.BytesIO(blob))
    assert im.format == "WEBP" and im.mode == mode and im.size == (px.shape[1], px.shape[0])
    assert np.array_equal(np.asarray(im), want)
    if not literal:
        return None
    d = webp_literal.decode(blob)
    assert d["alpha_used"] == (1 if mode == "RGBA" else 0)
    rgba = want if want.shape[2] == 4 else np.dstack([want, np.full(want.shape[:2] + (1,), 255, np.uint8)])
    assert np.array_equal(d["pixels"], rgba)
    return d


def table_inputs():
    """The three inputs of DESIGN.md 3.10's size table, RGBA."""
    root = os.path.join(ROOT, "tests", "golden")
    photo = np.asarray(Image.open(os.path.join(root, "smart_crop.jpg")).convert("RGB").resize((200, 150)))
    ramp = np.broadcast_to((np.arange(200) * 255 // 199).astype(np.uint8)[None, :, None], (150, 200, 1))
    square = np.asarray(Image.open(os.path.join(root, "square-opaque-200.png")).convert("RGBA"))
    synth = np.dstack([synth_rgb(160, 120, 3), np.full((120, 160, 1), 255, np.uint8)])
    return {"photo": np.ascontiguousarray(np.dstack([photo, ramp])), "square": np.ascontiguousarray(square),
            "synth": np.ascontiguousarray(synth)}


def pillow_png(px, **kw):
    b = io.BytesIO()
    Image.fromarray(px).save(b, "PNG", **kw)
    return len(b.getvalue())


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_bound_is_pixels_plus_a_constant_and_covers_noise(c):
    consts = set()
    for w, h in BOUND_GEOMETRIES:
        bound = webp_encode_bound(w, h, c)
        assert 0 < bound - w * h * c <= 1024
        consts.add(bound - w * h * c)
        if max(w, h) <= 333:
            f = webp_encode_host_form(channels(content("noise", w, h), c))
            assert len(f) <= bound, (w, h, c)
    assert len(consts) == 1  # the fallback form's header does not depend on the geometry


def test_bound_rejects_bad_arguments():
    n = L.ctypes.c_size_t()
    f = L.lib().fi_webp_encode_bound
    ref = L.ctypes.byref(n)
    for c in (1, 2, 3, 4):
        assert f(10, 10, c, ref) == L.FI_OK and n.value > 10 * 10 * c
    for c in (0, 5, -1):
        assert f(10, 10, c, ref) == L.FI_EINVAL
    for w, h in ((0, 10), (10, 0), (-1, 10)):
        assert f(w, h, 3, ref) == L.FI_EINVAL
    assert f(16384, 16384, 4, ref) == L.FI_OK
    assert f(16385, 1, 4, ref) == L.FI_EUNSUPPORTED
    assert f(1, 16385, 1, ref) == L.FI_EUNSUPPORTED
    assert f(10, 10, 3, None) == L.FI_EINVAL


def test_host_form_rejects_bad_arguments():
    f = L.lib().fi_debug_webp_encode_host
    px = np.zeros((4, 4, 4), np.uint8)
    out = np.zeros(4096, np.uint8)
    n = L.ctypes.c_size_t()

    def call(w=4, h=4, c=4, stride=16, pred=-1, cap=4096):
        return f(px.ctypes.data, w, h, c, stride, pred, out.ctypes.data, cap, L.ctypes.byref(n))

    assert call() == L.FI_OK and 0 < n.value <= webp_encode_bound(4, 4, 4)
    need = n.value
    assert call(c=5) == L.FI_EINVAL and call(c=0) == L.FI_EINVAL
    assert call(w=0) == L.FI_EINVAL and call(h=0) == L.FI_EINVAL
    assert call(pred=14) == L.FI_EINVAL and call(pred=-2) == L.FI_EINVAL
    assert call(stride=15) == L.FI_EINVAL
    assert call(w=16385, stride=16385 * 4) == L.FI_EUNSUPPORTED
    out[:] = 0xA5
    assert call(cap=need - 1) == L.FI_ENOMEM and n.value == need
    assert (out == 0xA5).all()  # nothing is written, let alone past the capacity


def test_pipeline_turns_down_gpu_webp_without_gpu_encode():
    from flyimg_amd.codec import CodecPipeline

    with pytest.raises(ValueError):
        CodecPipeline(None, gpu_webp=True)


@pytest.fixture(scope="module")
def driver():
    hipcc = _compiler("hipcc")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "webp_write")
        subprocess.run([hipcc, "-std=c++17", "-fno-gpu-sanitize", *SAN, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests/native/webp_write_driver.cpp"),
                        os.path.join(ROOT, "flyimg_amd/csrc/fi_webp_write.cpp"), "-o", exe],
                       check=True, capture_output=True, timeout=300)

        def run(lines):
            r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True,
                               timeout=300, env=ENV)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
            assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
            out = r.stdout.split("\n")
            assert f"DONE {len(lines)}" in out
            return out[:len(lines)]

        run.dir = d
        yield run


def _driver_encode(driver, cases):
    """cases: (array of rows incl. padding, w, h, c, stride, predictor, cap) -> [(rc, out_len, file bytes or None)]"""
    lines = []
    for k, (buf, w, h, c, stride, pred, cap) in enumerate(cases):
        ip, op = os.path.join(driver.dir, f"in{k}.bin"), os.path.join(driver.dir, f"out{k}.webp")
        with open(ip, "wb") as f:
            f.write(np.ascontiguousarray(buf).tobytes())
        if os.path.exists(op):
            os.remove(op)
        lines.append(f"enc {w} {h} {c} {stride} {pred} {cap} {ip} {op}")
    res = []
    for k, line in enumerate(driver(lines)):
        tag, rc, n = line.split()
        assert tag == "ENC"
        op = os.path.join(driver.dir, f"out{k}.webp")
        blob = None
        if int(rc) == 0:
            with open(op, "rb") as f:
                blob = f.read()
            assert len(blob) == int(n)
        res.append((int(rc), int(n), blob))
    return res


@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_round_trip_library_and_sanitised_driver(driver, w, h):
    cases, files = [], []
    for c in (1, 2, 3, 4):
        for name in CONTENTS:
            px = channels(content(name, w, h), c)
            f = webp_encode_host_form(px)
            assert len(f) <= webp_encode_bound(w, h, c)
            check_file(f, px)
            files.append(f)
            cases.append((px, w, h, c, w * c, -1, -1))
    for (rc, n, blob), f in zip(_driver_encode(driver, cases), files):
        assert rc == 0 and blob == f


def test_driver_strided_source_and_capacity(driver):
    w, h, c = 37, 21, 3
    px = channels(content("synth", w, h), c)
    stride = w * c + 13
    buf = np.full((h, stride), 0xEE, np.uint8)
    buf[:, :w * c] = px.reshape(h, w * c)
    buf = buf.ravel()[:(h - 1) * stride + w * c]  # the last row ends with its pixels: nothing behind them is read
    f = webp_encode_host_form(px)
    (rc, n, blob), (rc2, n2, _), (rc3, n3, blob3) = _driver_encode(driver, [
        (buf, w, h, c, stride, -1, -1), (buf, w, h, c, stride, -1, len(f) - 1), (buf, w, h, c, stride, -1, len(f))])
    assert rc == 0 and blob == f
    assert rc2 == L.FI_ENOMEM and n2 == len(f)
    assert rc3 == 0 and blob3 == f


@pytest.mark.parametrize("name", ["gradient", "noise"])
def test_every_predictor(driver, name):
    w, h = 37, 53
    px = content(name, w, h)
    cases = []
    sizes = {}
    for pred in list(range(14)) + [-1]:
        f = webp_encode_host_form(px, pred)
        d = check_file(f, px)
        if d["transforms"]:  # (noise may take the fallback form: no predictor at all)
            assert d["transforms"] == [2, 0]
            assert d["modes"].shape == (4, 3)
            if pred >= 0:
                assert (d["modes"] == pred).all()
        sizes[pred] = f
        cases.append((px, w, h, 4, w * 4, pred, -1))
        if pred == -1 and name == "gradient":
            assert d["transforms"] == [2, 0] and len(np.unique(d["modes"])) >= 2
    for (rc, n, blob), pred in zip(_driver_encode(driver, cases), list(range(14)) + [-1]):
        assert rc == 0 and blob == sizes[pred]
    if name == "gradient":
        assert len(sizes[-1]) <= len(sizes[0])  # the per-block choice is no worse than no prediction


def test_flat_image_is_tiny_and_made_of_matches():
    for c in (1, 2, 3, 4):
        px = channels(content("flat", 200, 200), c)
        f = webp_encode_host_form(px)
        assert len(f) < 100
        d = check_file(f, px)
        st = d["stats"]
        assert st["matches"] > 0 and st["literals"] + sum(st["lengths"]) == 200 * 200
        assert max(st["lengths"]) <= 4096 and st["forms"]["green"] == "normal"  # a literal plus length symbols
        # constant channels -- alpha where the source has none, red and blue of gray after subtract-green --
        # are single-symbol; the others hold pixel (0, 0)'s residual against (255, 0, 0, 0) and zeros
        constant = {1: ("red", "blue", "alpha"), 2: ("red", "blue"), 3: ("alpha",), 4: ()}[c]
        for k in ("red", "blue", "alpha"):
            if k in constant:
                assert st["forms"][k] == "simple1" and st["used"][k] == 1
            else:
                assert st["forms"][k] == "simple2" and st["used"][k] == 2


def test_one_pixel():
    for c in (1, 2, 3, 4):
        px = channels(content("noise", 1, 1), c)
        f = webp_encode_host_form(px)
        d = check_file(f, px)
        assert d["stats"]["literals"] == 1 and d["stats"]["matches"] == 0 and len(f) < 60
        assert all(v == "simple1" for v in d["stats"]["forms"].values())


def test_two_colours_take_simple_two_symbol_codes():
    # predictor 0: a residual is the pixel minus (255, 0, 0, 0), so opaque black leaves zeros -- as do row 0 and
    # column 0, which predict from L and T whatever the mode and are all black here
    pick = np.random.default_rng(8).integers(0, 2, (16, 16))
    pick[0, :] = pick[:, 0] = 0
    colours = np.array([[0, 0, 0, 255], [200, 100, 50, 128]], np.uint8)
    px = colours[pick]
    f = webp_encode_host_form(px, 0)
    d = check_file(f, px)
    st = d["stats"]
    for k in ("red", "blue", "alpha"):
        assert st["forms"][k] == "simple2" and st["used"][k] == 2


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


def test_code_builder_on_hard_histograms(driver):
    rng = np.random.default_rng(3)
    one = [0] * 280
    one[65] = 9
    two = [0] * 280
    two[0], two[256] = 1000, 1
    low_two = [0] * 256
    low_two[1], low_two[200] = 5, 7
    cases = [one, two, low_two, [7] * 280, _fib(40) + [0] * 240, [0] * 240 + _fib(40)[::-1], [0] * 40, [0] * 39 + [3],
             [1] * 279 + [32768], list(map(int, rng.integers(0, 3, 280))), list(map(int, rng.integers(1, 40000, 256))),
             [2 ** k for k in range(30)] + [0] * 10, [1] * 256 + [0] * 24]
    out = driver(["code %d %s" % (len(f), " ".join(map(str, f))) for f in cases])
    for k, (f, line) in enumerate(zip(cases, out)):
        parts = line.split()
        assert parts[0] == "CODE"
        bits, ent = int(parts[1]), [tuple(map(int, e.split(":"))) for e in parts[3:]]
        br = webp_literal.Bits(bytes.fromhex(parts[2]))
        code = webp_literal.read_code(br, len(f))  # (raises on an incomplete code or one deeper than 15 bits)
        assert br.pos == bits, k
        used = [s for s, v in enumerate(f) if v]
        assert code.used == (used or [0]), k
        for s in used:  # the table the emitter uses is the code the stream declares
            l, rev = ent[s]
            if len(used) == 1:
                assert l == 0
                continue
            assert l == code.lengths[s] and l <= 15
            assert code.table[(l, int(format(rev, f"0{l}b")[::-1], 2))] == s
        for i in used:  # a more frequent symbol never has the longer code
            for j in used:
                if f[i] > f[j]:
                    assert code.lengths[i] <= code.lengths[j], (k, i, j)
    forms = [webp_literal.read_code(webp_literal.Bits(bytes.fromhex(l.split()[2])), len(f)).form
             for f, l in zip(cases, out)]
    assert forms[:4] == ["simple1", "normal", "simple2", "normal"] and forms[6] == "simple1"
    depth = max(webp_literal.read_code(webp_literal.Bits(bytes.fromhex(out[4].split()[2])), 280).lengths)
    assert depth == 15  # the limit acts: 40 Fibonacci counts are 39 deep without it


def test_sizes_against_pillow_png():
    t = table_inputs()
    files = {k: webp_encode_host_form(v) for k, v in t.items()}
    for k, v in t.items():
        check_file(files[k], v, literal=False)
        print(k, len(files[k]), pillow_png(v), pillow_png(v, compress_level=1))
    assert len(files["photo"]) <= pillow_png(t["photo"])
    assert len(files["synth"]) <= pillow_png(t["synth"])
    assert len(files["square"]) <= pillow_png(t["square"], compress_level=1)
