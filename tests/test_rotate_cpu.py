"""CPU: -rotate by any integer angle with -background (the opt-in shear
rotation) -- the literal restatement's own properties
(tests/rotate_literal.py), the host planner against it (fi_debug_rotate with no
context, fi_plan with FI_OP_ROTATE_SHEAR / FI_OP_BACKGROUND), the ABI layout, the
option surface, and the kernel's per-pixel procedure run on the host
(fi_debug_rotate_host) against the literal, bit for bit."""
import ctypes
import math

import numpy as np
import pytest

from flyimg_amd import _lib as L
from flyimg_amd.processor import ExecFailedException, ImageProcessor, OptionsBag, parse_background
from flyimg_amd.runtime import Op, _fill, plan, plan_bytes, rotate_q16_host, rotated_size
from tests import rotate_literal as RL
from tests.test_plan_cpu import _batch

WHITE = (65535, 65535, 65535)


def _bg16(rgb):
    return [257 * ((rgb >> 16) & 255), 257 * ((rgb >> 8) & 255), 257 * (rgb & 255)]


def _random(w, h, ch, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 65536, (h, w, ch) if ch > 1 else (h, w), dtype=np.uint16)


def _checker(w, h, ch):
    yy, xx = np.mgrid[0:h, 0:w]
    q = (((yy + xx) & 1) * 65535).astype(np.uint16)
    return np.repeat(q[:, :, None], ch, 2) if ch > 1 else q


# --- the literal itself -----------------------------------------------------------
@pytest.mark.parametrize("deg", [0, 90, 180, 270, -90, 360, 450, -180])
def test_literal_multiples_of_90_are_rot90(deg):
    img = _random(7, 5, 3, 3)
    out, ok = RL.rotate(img, deg, WHITE)
    assert ok and np.array_equal(out, np.rot90(img, -(deg // 90) % 4))


@pytest.mark.parametrize("deg", [1, -7, 30, -44, 45, -45, 46, 135, 200])
def test_literal_constant_image_and_value_range(deg):
    for w, h in ((8, 8), (13, 9), (9, 13), (41, 31)):
        c, b = 40000, 12345
        img = np.full((h, w), c, np.uint16)
        same, ok = RL.rotate(img, deg, (c,))
        assert ok and (same == c).all(), (w, h, deg)
        out, ok = RL.rotate(img, deg, (b,))
        assert ok and out.min() >= min(b, c) and out.max() <= max(b, c), (w, h, deg)
        _, sx, _ = RL.reduce_angle(deg)
        if abs(math.degrees(math.atan(-sx)) * 2) >= 10 and min(w, h) >= 8:
            corners = [out[0, 0], out[0, -1], out[-1, 0], out[-1, -1]]
            assert all(int(v) == b for v in corners), (w, h, deg, corners)


def _rot_cw(theta_deg, v):
    """clockwise on the screen (y down) by theta"""
    t = math.radians(theta_deg)
    return (v[0] * math.cos(t) - v[1] * math.sin(t), v[0] * math.sin(t) + v[1] * math.cos(t))


@pytest.mark.parametrize("deg", [30, -30, 45, -45, 10, 100, 200])
def test_literal_impulse_mass_and_centroid(deg):
    """A single pixel on black, black background: every shear splits a pixel
    between two neighbours with weights that sum to one (mass conserved up to
    the rounding of each of the at most 2 + 4 + 8 samples written: 3 units per
    shear), and places it within half a sample of its continuous position, so
    the centroid lands within 1.5 px of centre + Rot_cw(theta) (p - centre) --
    a bound a wrong sign convention misses by many pixels."""
    w, h, px, py, val = 41, 31, 30, 8, 60000
    img = np.zeros((h, w), np.uint16)
    img[py, px] = val
    out, ok = RL.rotate(img, deg, (0,))
    assert ok
    o = out.astype(np.float64)
    assert abs(o.sum() - val) <= 3 * 3, o.sum()
    yy, xx = np.mgrid[0:out.shape[0], 0:out.shape[1]]
    cx, cy = (o * (xx + 0.5)).sum() / o.sum(), (o * (yy + 0.5)).sum() / o.sum()
    dx, dy = _rot_cw(deg, (px + 0.5 - w / 2.0, py + 0.5 - h / 2.0))
    ex, ey = out.shape[1] / 2.0 + dx, out.shape[0] / 2.0 + dy
    print(f"{deg}: centroid ({cx:.2f}, {cy:.2f}) analytic ({ex:.2f}, {ey:.2f})")
    assert math.hypot(cx - ex, cy - ey) <= 1.5, (deg, (cx, cy), (ex, ey))


# --- the planner against the literal ---------------------------------------------------
SIZES = [(w, h) for w in range(1, 25) for h in range(1, 25)] + [(400, 400), (500, 281), (300, 250)]
ANGLES = [1, -7, 30, -44, 45, -45, 46, 135, 181, 271, -405]


def _plan_image(w, h, deg, flags=0, background=None, channels=3):
    img = L.FiImage()
    img.src_w, img.src_h, img.src_stride, img.src_channels = w, h, w * channels, channels
    img.flags = L.FI_OP_THUMBNAIL | L.FI_OP_ROTATE | flags
    img.rotate = deg
    if background is not None:
        img.flags |= L.FI_OP_BACKGROUND
        img.background = background
    rc = L.lib().fi_plan(ctypes.byref(img), 1)
    return rc, img


@pytest.mark.parametrize("deg", ANGLES)
def test_planner_sizes_and_containment_match_literal(deg):
    """fi_debug_rotate(NULL, ...) and fi_plan with FI_OP_ROTATE_SHEAR give the
    literal's out_w x out_h and reject exactly the images on which IM's scans
    would index outside the canvas."""
    rejected = 0
    for w, h in SIZES:
        ow, oh, ok = RL.rotated_size(w, h, deg)
        want = (ow, oh) if ok else None
        assert rotated_size(w, h, deg) == want, (w, h, deg)
        rc, img = _plan_image(w, h, deg, L.FI_OP_ROTATE_SHEAR)
        if ok:
            assert rc == L.FI_OK and (img.out_w, img.out_h, img.out_channels, img.out_stride) == (ow, oh, 3, 3 * ow)
        else:
            rejected += 1
            assert rc == L.FI_EUNSUPPORTED and b"canvas" in L.lib().fi_last_error()
        # without the flag: rejected exactly as before
        rc, _ = _plan_image(w, h, deg)
        assert rc == L.FI_EUNSUPPORTED and b"multiples of 90" in L.lib().fi_last_error()
    assert rejected < len(SIZES) // 4, rejected  # tall, narrow images only (none at small angles)


def test_planner_known_sizes():
    assert rotated_size(400, 400, -45) == (566, 566)  # BASELINE's r_-45,w_400,h_400
    assert RL.rotated_size(400, 400, -45) == (566, 566, True)
    assert rotated_size(5, 64, -30) is None
    # the literal's full scan agrees with its line-by-line verdict where the latter says no
    _, ok = RL.rotate(np.zeros((64, 5), np.uint16), -30, (0,))
    assert not ok


def test_literal_scan_verdict_equals_its_size_verdict():
    for w, h in [(w, h) for w in (1, 2, 3, 5, 8, 13) for h in (1, 2, 4, 7, 12, 20, 24)]:
        for deg in (7, -30, 45, 135):
            out, ok = RL.rotate(np.zeros((h, w), np.uint16), deg, (0,))
            ow, oh, ok2 = RL.rotated_size(w, h, deg)
            assert ok == ok2, (w, h, deg)
            if ok:
                assert out.shape == (oh, ow)


@pytest.mark.parametrize("deg", [0, 90, -90, 180, 270, 450])
def test_flag_with_multiple_of_90_plans_as_before(deg):
    rc0, a = _plan_image(333, 777, deg)
    rc1, b = _plan_image(333, 777, deg, L.FI_OP_ROTATE_SHEAR, background=0x123456)
    assert rc0 == rc1 == L.FI_OK
    assert (a.out_w, a.out_h, a.out_channels, a.out_stride) == (b.out_w, b.out_h, b.out_channels, b.out_stride)


def test_flag_with_multiple_of_90_uploads_the_same_blob():
    """the batch planner emits the same bytes for r_270 with and without the
    opt-in flags (fi_debug_host_plan's digest of the upload blob)"""
    lib = L.lib()
    digests = []
    try:
        for extra, bg in ((0, None), (L.FI_OP_ROTATE_SHEAR | L.FI_OP_BACKGROUND, 0x336699)):
            lib.fi_debug_host_plan(None, 0, 0, None)
            arr = _batch([(333, 777, "h_100,r_270"), (640, 480, "w_200,r_90")])
            for a in arr:
                a.flags |= extra
                if bg is not None:
                    a.background = bg
            ms = (ctypes.c_double * 7)()
            L.check(lib.fi_debug_host_plan(arr, len(arr), 1, ms))
            r = (ctypes.c_double * 7)()
            L.check(lib.fi_debug_host_plan(None, 3, 0, r))
            digests.append(tuple(r[:3]))
    finally:
        lib.fi_debug_host_plan(None, 0, 0, None)
    assert digests[0] == digests[1]


def test_sheared_batch_plans_on_the_host():
    """plan_batch / place_batch with sheared images beside others: every image plans"""
    lib = L.lib()
    lib.fi_debug_host_plan(None, 0, 0, None)
    try:
        arr = _batch([(1920, 1080, "w_400,h_400,c_1"), (1920, 1080, "w_400,h_400,c_1,r_90"), (600, 400, "w_96")] * 2)
        for k in (0, 3):
            arr[k].flags |= L.FI_OP_ROTATE | L.FI_OP_ROTATE_SHEAR
            arr[k].rotate = -45
            arr[k].dst_capacity = 566 * 566 * 3
        ms = (ctypes.c_double * 7)()
        L.check(lib.fi_debug_host_plan(arr, len(arr), 1, ms))
    finally:
        lib.fi_debug_host_plan(None, 0, 0, None)


def test_plan_bytes_adds_the_stage():
    plain = Op(400, 400, L.FI_OP_THUMBNAIL | L.FI_GEOM_FILL | L.FI_OP_EXTENT)
    rot = Op(400, 400, plain.flags | L.FI_OP_ROTATE | L.FI_OP_ROTATE_SHEAR, rotate=-45)
    a, b = plan_bytes([(1920, 1080, plain), (1920, 1080, rot)])
    # the integral Q16 image read once, and the larger output written
    assert b - a == 400 * 400 * 3 * 2 + (566 * 566 - 400 * 400) * 3


# --- ABI ------------------------------------------------------------------------------------
def test_fi_image_layout():
    assert ctypes.sizeof(L.FiImage) == 184
    assert L.FiImage.background.offset == 52 and L.FiImage.background.size == 4
    want = {"src": 0, "src_w": 8, "src_h": 12, "src_stride": 16, "src_channels": 20, "target_w": 24, "target_h": 28,
            "flags": 32, "gravity": 36, "rotate": 40, "smartcrop_w": 44, "smartcrop_h": 48, "dst": 56,
            "dst_capacity": 64, "out_w": 72, "out_h": 76, "out_channels": 80, "out_stride": 84, "crop_x": 88,
            "crop_y": 92, "crop_w": 96, "crop_h": 100, "crop_score": 104, "status": 112, "n_candidates": 116,
            "unsharp": 120, "sharpen": 152, "blur": 168}
    for name, off in want.items():
        assert getattr(L.FiImage, name).offset == off, name
    assert L.lib().fi_abi_version() == 2
    assert (L.FI_OP_ROTATE_SHEAR, L.FI_OP_BACKGROUND) == (1 << 14, 1 << 15)


# --- option surface ------------------------------------------------------------------------
def test_to_op_default_still_rejects():
    with pytest.raises(ExecFailedException):
        ImageProcessor(OptionsBag("w_200,r_-45"), 400, 300).to_op()
    with pytest.raises(ExecFailedException):
        ImageProcessor(OptionsBag("w_200,bg_red"), 400, 300).to_op()


def test_to_op_opt_in():
    op = ImageProcessor(OptionsBag("w_200,r_-45,bg_#999999"), 400, 300, shear_rotate=True).to_op()
    assert op.flags & L.FI_OP_ROTATE and op.flags & L.FI_OP_ROTATE_SHEAR
    assert op.rotate == -45 and op.background == 0x999999
    img = L.FiImage()
    _fill(img, op)
    assert img.flags & L.FI_OP_BACKGROUND and img.background == 0x999999
    assert plan(400, 300, op) == RL.rotated_size(200, 150, -45)[:2] + (3,)
    with pytest.raises(ExecFailedException):
        ImageProcessor(OptionsBag("w_200,r_12.5"), 400, 300, shear_rotate=True).to_op()
    plain = ImageProcessor(OptionsBag("w_200"), 400, 300, shear_rotate=True).to_op()
    assert plain.background == -1 and not plain.flags & (L.FI_OP_ROTATE | L.FI_OP_ROTATE_SHEAR)
    img = L.FiImage()
    _fill(img, plain)
    assert not img.flags & L.FI_OP_BACKGROUND
    # Op's new field is the last one: positional construction is unchanged
    assert Op(1, 2, 3, 4, 5, 6, 7, (0, 1, 1, 0), (0, 1), (0, 1), 0x10203).background == 0x10203


@pytest.mark.parametrize("text,want", [
    ("#999999", 0x999999), ("#abc", 0xAABBCC), ("#ABCDEF", 0xABCDEF), ("rgb(1,2,3)", 0x010203),
    ("rgb( 255 , 0,128 )", 0xFF0080), ("white", 0xFFFFFF), ("Black", 0), ("RED", 0xFF0000), ("lime", 0x00FF00),
    ("blue", 0xFF), ("yellow", 0xFFFF00), ("cyan", 0x00FFFF), ("aqua", 0x00FFFF), ("magenta", 0xFF00FF),
    ("fuchsia", 0xFF00FF)])
def test_background_parse_table(text, want):
    assert parse_background(text) == want


@pytest.mark.parametrize("text", ["#9999", "#99999999", "rgba(1,2,3,0.5)", "rgb(256,0,0)", "rgb(10%,0,0)",
                                  "transparent", "none", "green", "#ggg", "hsl(1,2,3)", "rgb(1,2)"])
def test_background_rejections(text):
    with pytest.raises(ExecFailedException, match="-background .* is not on the GPU path"):
        parse_background(text)


def test_fi_plan_rejections():
    S = L.FI_OP_ROTATE_SHEAR
    rc, _ = _plan_image(64, 48, 30, S, channels=4)
    assert rc == L.FI_EUNSUPPORTED and b"RGBA" in L.lib().fi_last_error()
    rc, _ = _plan_image(64, 48, 90, S, background=0xFF0000, channels=4)  # -background with RGBA, no shear
    assert rc == L.FI_EUNSUPPORTED and b"RGBA" in L.lib().fi_last_error()
    rc, _ = _plan_image(64, 48, 30, S | L.FI_OP_MONOCHROME)
    assert rc == L.FI_EUNSUPPORTED and b"monochrome" in L.lib().fi_last_error()
    rc, _ = _plan_image(64, 48, 30, S | L.FI_OP_GRAY, background=0xFF0000)
    assert rc == L.FI_EUNSUPPORTED and b"Gray" in L.lib().fi_last_error()
    rc, img = _plan_image(64, 48, 30, S | L.FI_OP_GRAY, background=0x808080)
    assert rc == L.FI_OK and img.out_channels == 1
    # -background without a shear rotation: accepted, no effect
    rc, img = _plan_image(64, 48, 90, 0, background=0xFF0000)
    assert rc == L.FI_OK and (img.out_w, img.out_h) == (48, 64)


# --- the kernel's procedure on the host ----------------------------------------------------
HOST_SHAPES = [(1, 1), (2, 3), (3, 2), (7, 5), (16, 16), (17, 33), (33, 17), (40, 30)]
HOST_ANGLES = [1, -1, 7, -30, 44, -44, 45, -45, 46, 89, 91, 135, -135, 179, 181, 271, 359, 405]


@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("shape", HOST_SHAPES, ids=[f"{w}x{h}" for w, h in HOST_SHAPES])
def test_host_model_is_the_literal(shape, ch):
    """fi_debug_rotate_host runs the device kernel's per-pixel code on the CPU:
    Q16 and 8-bit outputs equal the literal's, bit for bit"""
    w, h = shape
    k = 0
    for deg in HOST_ANGLES:
        for bg in (0xFFFFFF, 0x000000, 0x123456 if ch == 3 else 0x565656)[k % 3:][:1]:
            img = _random(w, h, ch, 7 * w + h + 1000 + deg) if k % 2 else _checker(w, h, ch)
            k += 1
            ref, ok = RL.rotate(img, deg, _bg16(bg))
            assert ok, (shape, deg)
            q, b = rotate_q16_host(img, deg, bg)
            assert q.shape == ref.shape and np.array_equal(q, ref), (shape, deg, hex(bg))
            assert np.array_equal(b, RL.q2c(ref))
