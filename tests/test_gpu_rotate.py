"""GPU: -rotate by any integer angle with -background (opt-in shear rotation,
fi_rotate.hip).

  * the kernel through ``Context.rotate_q16`` against tests/rotate_literal.py on
    the identical Q16 input: bit for bit, Q16 and 8-bit outputs;
  * the pipeline (host and device-resident entry points) against the literal
    applied to the oracle's resized Q16 image: within 1, >= 98 % exact;
  * the stage feeding the convolutions, the smart-crop stage and its apply;
  * mixed batches: images without a shear keep their bytes.
"""
import dataclasses

import numpy as np
import pytest

from flyimg_amd import _lib as L
from flyimg_amd.processor import ImageProcessor, OptionsBag, process_new_image
from flyimg_amd.runtime import Context, rotate_q16_host
from flyimg_amd.synth import synth_rgb
from oracle import oracle as orc
from tests import rotate_literal as RL

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 3), (3, 2), (7, 5), (16, 16), (17, 33), (33, 17), (40, 30), (64, 48)]
ANGLES = [1, -1, 7, -30, 44, -44, 45, -45, 46, 89, 91, 135, -135, 179, 181, 271, 359, 405]
# every angle twice, every shape at least four times
PAIRS = ([(SHAPES[j % 9], ANGLES[j]) for j in range(18)] + [(SHAPES[(j + 4) % 9], ANGLES[j]) for j in range(18)]
         + [((64, 48), 45), ((64, 48), -30), ((1, 1), 45), ((40, 30), 91)])
assert len(set(PAIRS)) == len(PAIRS) == 40
BACKGROUNDS = [0xFFFFFF, 0x000000, 0x123456]


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def src():
    return synth_rgb(600, 400, 0xA11CE)


def _bg16(rgb):
    return [257 * ((rgb >> 16) & 255), 257 * ((rgb >> 8) & 255), 257 * (rgb & 255)]


def _content(w, h, ch, k):
    if k % 2:
        q = np.random.default_rng(1000 + k).integers(0, 65536, (h, w, ch), dtype=np.uint16)
    else:  # 0 / 65535 checkerboard: clamps and rounding ties
        yy, xx = np.mgrid[0:h, 0:w]
        q = np.repeat((((yy + xx) & 1) * 65535).astype(np.uint16)[:, :, None], ch, 2)
    return q if ch == 3 else np.ascontiguousarray(q[:, :, 0])


@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("k", range(len(PAIRS)), ids=[f"{w}x{h}@{a}" for (w, h), a in PAIRS])
def test_kernel_is_the_literal(ctx, k, ch):
    (w, h), deg = PAIRS[k]
    bg = BACKGROUNDS[k % 3]
    if ch == 1:  # Gray takes a gray background
        bg = (bg & 255) * 0x010101
    q = _content(w, h, ch, k)
    ref, ok = RL.rotate(q, deg, _bg16(bg))
    assert ok, "every pair here stays on IM's canvas"
    got16, got8 = ctx.rotate_q16(q, deg, bg)
    assert got16.shape == ref.shape
    assert np.array_equal(got16, ref), (int((got16 != ref).sum()), int(np.abs(got16.astype(int) - ref).max()))
    assert np.array_equal(got8, RL.q2c(ref))


def test_kernel_rejects_what_leaves_the_canvas(ctx):
    with pytest.raises(L.FiError) as e:
        ctx.rotate_q16(np.zeros((64, 5, 3), np.uint16), -30)
    assert e.value.code == L.FI_EUNSUPPORTED


def test_kernel_multi_tile_equals_host_model(ctx):
    """more than one tile in x and y, a width that is no multiple of 4 px, rows
    at every dword phase: the kernel equals its own per-pixel procedure run on
    the host (which the CPU suite holds to the literal)"""
    q = np.random.default_rng(5).integers(0, 65536, (203, 301, 3), dtype=np.uint16)
    for deg, bg in ((-45, 0x123456), (20, 0xFFFFFF)):
        got16, got8 = ctx.rotate_q16(q, deg, bg)
        ref16, ref8 = rotate_q16_host(q, deg, bg)
        assert got16.shape[1] > 256 and got16.shape[0] > 4
        assert np.array_equal(got16, ref16) and np.array_equal(got8, ref8)
    g16, g8 = ctx.rotate_q16(np.ascontiguousarray(q[:, :, 1]), 33, 0x808080)
    r16, r8 = rotate_q16_host(np.ascontiguousarray(q[:, :, 1]), 33, 0x808080)
    assert np.array_equal(g16, r16) and np.array_equal(g8, r8)


# --- pipeline ---------------------------------------------------------------------------
def _op(options, w, h):
    return ImageProcessor(OptionsBag(options), w, h, shear_rotate=True).to_op()


def _device_run(ctx, images, ops):
    ptrs = [ctx.malloc(im.nbytes) for im in images]
    try:
        for p, im in zip(ptrs, images):
            ctx.h2d(p, im)
        views = [(p, im.shape[1], im.shape[0], im.strides[0]) for p, im in zip(ptrs, images)]
        outs, recs, rc = ctx.process_device_views(views, ops)
    finally:
        for p in ptrs:
            ctx.free(p)
    return outs, recs, rc


def _oracle_q16(src, options):
    """the oracle's resized Q16 image for the w_ / rz_ / c_ part of `options`"""
    bag = OptionsBag(options)
    w, c = int(bag.get_option("width")), bag.get_option("crop")
    thumb = not bag.get_option("resize")
    H, W = src.shape[:2]
    if c:
        hh = int(bag.get_option("height"))
        tw, th = orc.im_meta_geometry(W, H, w, hh, True, False)
        gx, gy = orc.im_gravity_offset(tw, th, w, hh)
        return orc.im_resize_q16(src, tw, th, thumbnail=thumb)[gy:gy + hh, gx:gx + w]
    tw, th = orc.im_meta_geometry(W, H, w, 0, False, True)
    return orc.im_resize_q16(src, tw, th, thumbnail=thumb)


PIPE = [("w_96,r_-45", -45, 0xFFFFFF), ("w_96,r_30,bg_#999999", 30, 0x999999), ("w_80,rz_1,r_135", 135, 0xFFFFFF)]


@pytest.fixture(scope="module")
def pipe_refs(src):
    """computed once: q2c(literal(oracle's resized Q16))"""
    refs = {}
    for options, deg, bg in PIPE:
        out, ok = RL.rotate(_oracle_q16(src, options), deg, _bg16(bg))
        assert ok
        refs[options] = RL.q2c(out)
    return refs


def _close(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    print(f"max diff {d.max()}, exact {(d == 0).mean():.4f}")
    assert d.max() <= 1
    assert (d == 0).mean() >= 0.98


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("options", [p[0] for p in PIPE])
def test_pipeline_matches_literal_on_oracle_q16(ctx, src, pipe_refs, options, entry):
    op = _op(options, 600, 400)
    run = ctx.process if entry == "host" else (lambda ims, ops: _device_run(ctx, ims, ops))
    outs, recs, rc = run([src], [op])
    L.check(rc)
    _close(outs[0], pipe_refs[options])


def test_pipeline_gray_route(ctx, src):
    options = "w_96,h_96,c_1,clsp_Gray,r_-20"
    q = _oracle_q16(src, options).astype(np.float64)
    # -colorspace Gray on the Q16 image (Rec709Luma, ClampToQuantum), then -rotate
    g = 0.212656 * q[:, :, 0] + 0.715158 * q[:, :, 1] + 0.072186 * q[:, :, 2]
    g16 = np.where(g <= 0, 0, np.where(g >= 65535.0, 65535, np.floor(g + 0.5))).astype(np.uint16)
    assert np.array_equal(RL.q2c(g16), orc.im_convert(src, 96, 96, orc.FLAG_THUMBNAIL | orc.FLAG_FILL | orc.FLAG_EXTENT
                                                       | orc.FLAG_GRAY))
    ref, ok = RL.rotate(g16, -20, (65535,))
    assert ok
    outs, recs, rc = ctx.process([src], [_op(options, 600, 400)])
    L.check(rc)
    assert recs[0].out_channels == 1
    _close(outs[0], RL.q2c(ref))


def test_baseline_rotate_row(ctx):
    """BASELINE.md's r_-45,w_400,h_400 through process_new_image"""
    big = synth_rgb(1920, 1080, 0x5EED)
    out, rec = process_new_image(ctx, "w_400,h_400,r_-45", big, shear_rotate=True)
    q = orc.im_resize_q16(big, 400, 225)
    ref16, ref8 = rotate_q16_host(q, -45, 0xFFFFFF)  # the kernel's procedure on the host (CPU suite: == literal)
    assert (rec.out_w, rec.out_h) == ref8.shape[1::-1] == RL.rotated_size(400, 225, -45)[:2]
    _close(out, ref8)
    assert (out[0, 0] == 255).all() and (out[-1, -1] == 255).all()
    with pytest.raises(Exception):
        process_new_image(ctx, "w_400,h_400,r_-45", big)


def test_rotation_feeds_the_convolutions(ctx, src):
    """w_96,r_-30,blr_1: the oracle's -blur on the GPU's own rotated Q16 (debug
    entry on the oracle's resized Q16), within 1"""
    outs, recs, rc = ctx.process([src], [_op("w_96,r_-30,blr_1", 600, 400)])
    L.check(rc)
    rot16, _ = ctx.rotate_q16(_oracle_q16(src, "w_96"), -30, 0xFFFFFF)
    ref = orc.im_convolve_q16(rot16, (0, 1, 1, 0.05, 0, 1, 1.0, 1.0), 4)
    assert outs[0].shape == ref.shape
    d = np.abs(outs[0].astype(np.int16) - ref.astype(np.int16))
    print(f"max diff {d.max()}, exact {(d == 0).mean():.4f}")
    assert d.max() <= 1


def test_rotation_feeds_smartcrop_and_apply(ctx, src):
    op = _op("w_200,r_-45,smc_1", 600, 400)
    no_apply = dataclasses.replace(op, flags=op.flags & ~L.FI_OP_SMARTCROP_APPLY)
    outs, recs, rc = ctx.process([src, src], [no_apply, op])
    L.check(rc)
    rotated, rec = outs[0], recs[0]
    assert rotated.shape[1::-1] == RL.rotated_size(200, 133, -45)[:2]
    t = orc.sc_crop(rotated, 100, 100)["top_crop"]
    assert (rec.crop_x, rec.crop_y, rec.crop_w, rec.crop_h) == (t["x"], t["y"], t["width"], t["height"])
    H, W = rotated.shape[:2]
    ow, oh = min(t["width"] + t["x"], W - t["x"]), min(t["height"] + t["y"], H - t["y"])
    assert np.array_equal(outs[1], rotated[t["y"]:t["y"] + oh, t["x"]:t["x"] + ow])


def test_mixed_batch_keeps_the_others_bytes(ctx, src):
    sheared, quarter, plain = _op("w_96,r_30,bg_#999999", 600, 400), _op("w_96,r_90", 600, 400), _op("w_120", 600, 400)
    for entry in (ctx.process, lambda ims, ops: _device_run(ctx, ims, ops)):
        outs, recs, rc = entry([src, src, src], [sheared, quarter, plain])
        L.check(rc)
        alone, _, rc = entry([src, src], [quarter, plain])
        L.check(rc)
        assert np.array_equal(outs[1], alone[0]) and np.array_equal(outs[2], alone[1])
        only, _, rc = entry([src], [sheared])
        L.check(rc)
        assert np.array_equal(outs[0], only[0])
    # the flag with r_90: the bytes of r_90 without it
    old = ImageProcessor(OptionsBag("w_96,r_90"), 600, 400).to_op()
    assert quarter.flags & L.FI_OP_ROTATE_SHEAR and not old.flags & L.FI_OP_ROTATE_SHEAR
    a, _, rc = ctx.process([src], [old])
    L.check(rc)
    b, _, rc = ctx.process([src], [quarter])
    L.check(rc)
    assert np.array_equal(a[0], b[0])
