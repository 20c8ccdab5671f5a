"""GPU JPEG decode through a view (fi_jpeg_decode_device_view,
k_jpeg_color_view): EXIF auto-orient and ExtractProcessor's rectangle applied
by the decoder's colour stage.  The reference is the host decode path:
ImageOps.exif_transpose of Pillow's decode, cropped -- exact equality
throughout."""
import io

import numpy as np
import pytest
from PIL import Image

from flyimg_amd import _lib as L
from flyimg_amd.codec import CodecPipeline
from flyimg_amd.processor import ExecFailedException
from flyimg_amd.runtime import Context

from . import _orient_files as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _oriented(px, o, **kw):
    """A file carrying EXIF orientation ``o`` (hand-built APP1 after JFIF)."""
    return F.splice(F.jpeg(px, **kw), F.exif_app1(o, le=o % 2 == 0))


def _same(got, ref, name):
    assert got is not None, name
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.array_equal(got, ref), f"{name}: {(got != ref).sum()} of {ref.size} values differ"


SAMPLINGS = {"444": dict(subsampling=0), "422": dict(subsampling=1), "420": dict(subsampling=2), "gray": None}
SIZES = [(1, 1), (7, 9), (17, 33), (33, 65)]


@pytest.mark.parametrize("sampling", list(SAMPLINGS))
def test_all_orientations_small_sizes(ctx, sampling):
    """1x1, 7x9, 17x33, 33x65 (tile edges, partial tiles, odd chroma sizes, the
    transposed partial tile) x the eight orientations, one batch per sampling."""
    kw = SAMPLINGS[sampling]
    blobs, views, names = [], [], []
    for (w, h) in SIZES:
        px = F.photo(w, h, gray=kw is None)
        for o in range(1, 9):
            blobs.append(_oriented(px, o, **(kw or {})))
            views.append((o, 0, 0, 0, 0))
            names.append(f"{sampling} {w}x{h} o{o}")
    outs = ctx.jpeg_decode_host(blobs, views=views)
    for blob, got, name in zip(blobs, outs, names):
        _same(got, F.reference(blob, mode="L" if kw is None else "RGB"), name)


def test_640x481_420_rotations(ctx):
    px = F.photo(640, 481)
    blobs = [_oriented(px, o, subsampling=2, quality=90) for o in (6, 8)]
    outs = ctx.jpeg_decode_host(blobs, views=[(6, 0, 0, 0, 0), (8, 0, 0, 0, 0)])
    for blob, got, o in zip(blobs, outs, (6, 8)):
        assert got.shape == (640, 481, 3)
        _same(got, F.reference(blob), f"640x481 o{o}")


def _rects(ow, oh):
    return {"inner": (1, 1, 31, 33), "last_pixel": (ow - 1, oh - 1, 1, 1), "right_bottom": (ow - 40, oh - 35, 40, 35),
            "full_row": (0, oh // 2, ow, 1), "full_column": (ow // 3, 0, 1, oh)}


def test_rectangles_97x61_420(ctx):
    px = F.photo(97, 61)
    blobs, views, names = [], [], []
    for o in (1, 3, 6, 7):
        blob = _oriented(px, o, subsampling=2)
        ow, oh = (61, 97) if o >= 5 else (97, 61)
        for name, r in _rects(ow, oh).items():
            blobs.append(blob)
            views.append((o,) + r)
            names.append(f"o{o} {name} {r}")
    outs = ctx.jpeg_decode_host(blobs, views=views)
    for blob, v, got, name in zip(blobs, views, outs, names):
        _same(got, F.reference(blob, v[1:]), name)


def _decode_raw(ctx, blobs, views, dims, pad, extra_rows=2, channels=0, progressive=False, fill=0xA5):
    """Decode into sentinel-filled buffers of (h + extra_rows) rows of w * c + pad bytes; the whole buffers."""
    strides = [w * c + pad for w, h, c in dims]
    sizes = [s * (h + extra_rows) for s, (w, h, c) in zip(strides, dims)]
    ptrs = [ctx.malloc(sz) for sz in sizes]
    try:
        for p, sz in zip(ptrs, sizes):
            ctx.h2d(p, np.full(sz, fill, np.uint8))
        status = ctx.jpeg_decode(blobs, ptrs, strides, channels=channels, progressive=progressive, views=views)
        return status, [ctx.d2h(p, sz).reshape(-1, s) for p, sz, s in zip(ptrs, sizes, strides)]
    finally:
        for p in ptrs:
            ctx.free(p)


def test_padding_and_trailing_rows_untouched(ctx):
    px = F.photo(97, 61)
    cases = [(1, (3, 5, 50, 40)), (2, (0, 0, 0, 0)), (6, (1, 1, 31, 33)), (5, (0, 0, 0, 0)), (8, (20, 64, 41, 33))]
    blobs = [_oriented(px, o, subsampling=2) for o, _ in cases]
    views = [(o,) + r for o, r in cases]
    dims = []
    for o, r in cases:
        ow, oh = (61, 97) if o >= 5 else (97, 61)
        dims.append((r[2] or ow, r[3] or oh, 3))
    status, bufs = _decode_raw(ctx, blobs, views, dims, pad=13)
    assert status == [0] * len(cases)
    for blob, v, (w, h, c), buf in zip(blobs, views, dims, bufs):
        rect = v[1:] if v[3] else None
        _same(buf[:h, :w * c].reshape(h, w, c), F.reference(blob, rect), str(v))
        assert (buf[:h, w * c:] == 0xA5).all(), f"{v}: row padding written"
        assert (buf[h:] == 0xA5).all(), f"{v}: rows after the rectangle written"


def test_gray_as_rgb_orientation_5(ctx):
    blob = _oriented(F.photo(33, 65, gray=True), 5)
    status, (buf,) = _decode_raw(ctx, [blob], [(5, 0, 0, 0, 0)], [(65, 33, 3)], pad=0, extra_rows=0, channels=3)
    assert status == [0]
    _same(buf.reshape(33, 65, 3), F.reference(blob, mode="RGB"), "gray as RGB o5")


def test_progressive_with_view(ctx):
    blob = _oriented(F.photo(97, 61), 6, subsampling=2, progressive=True)
    rect = (5, 7, 40, 70)
    got = ctx.jpeg_decode_host([blob], progressive=True, views=[(6,) + rect])[0]
    _same(got, F.reference(blob, rect), "progressive o6 rect")
    # without the flag the stream is the host's, view or not
    status, _ = _decode_raw(ctx, [blob], [(6,) + rect], [(40, 70, 3)], pad=0)
    assert status == [L.FI_EUNSUPPORTED]


def test_orientation_0_reads_the_file(ctx):
    px = F.photo(50, 30)
    o8 = F.pillow_oriented(px, 8, subsampling=2)
    xmp = F.splice(F.jpeg(px), F.xmp_app1(6))
    plain = F.jpeg(px)
    dims = [(30, 50, 3), (30, 50, 3), (50, 30, 3)]
    status, bufs = _decode_raw(ctx, [o8, xmp, plain], [(0, 0, 0, 0, 0)] * 3, dims, pad=0, extra_rows=0)
    assert status == [0, L.FI_EUNSUPPORTED, 0]
    _same(bufs[0].reshape(50, 30, 3), F.reference(o8), "orientation 0 on an orientation-8 file")
    assert F.reference(o8).shape == (50, 30, 3)
    _same(bufs[2].reshape(30, 50, 3), F.reference(plain), "orientation 0 on a plain file")
    assert (bufs[1] == 0xA5).all()  # the undetermined one is left to the host, untouched
    got = ctx.jpeg_decode_host([o8, xmp], views=[(0, 2, 3, 20, 40), (0, 0, 0, 0, 0)])
    _same(got[0], F.reference(o8, (2, 3, 20, 40)), "orientation 0 + rectangle")
    assert got[1] is None


def test_invalid_views_are_einval_per_image(ctx):
    blob = _oriented(F.photo(97, 61), 6, subsampling=2)  # oriented: 61 x 97
    bad = [(9, 0, 0, 0, 0), (-1, 0, 0, 0, 0), (6, -1, 0, 10, 10), (6, 0, -1, 10, 10), (6, 0, 0, 0, 10), (6, 0, 0, 10, 0),
           (6, 5, 0, 0, 0), (6, 0, 0, -3, 10), (6, 0, 0, 62, 10), (6, 52, 0, 10, 10), (6, 0, 88, 10, 10),
           (1, 0, 0, 61, 97), (6, 61, 0, 1, 1), (6, 0, 0, 2 ** 31 - 1, 1)]
    good = [(6, 0, 0, 61, 97), (6, 51, 87, 10, 10), (1, 0, 0, 97, 61)]
    views = bad + good
    dims = [(97, 97, 3)] * len(views)  # (large enough for any valid view)
    status, bufs = _decode_raw(ctx, [blob] * len(views), views, dims, pad=0, extra_rows=0)
    assert status == [L.FI_EINVAL] * len(bad) + [0] * len(good)
    for buf in bufs[:len(bad)]:
        assert (buf == 0xA5).all()
    plain = np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))
    for v, buf in zip(good, bufs[len(bad):]):
        w, h = v[3], v[4]
        got = buf.reshape(-1)
        rows = np.stack([got[r * 97 * 3:r * 97 * 3 + w * 3] for r in range(h)]).reshape(h, w, 3)
        ref = F.reference(blob, v[1:]) if v[0] == 6 else plain[v[2]:v[2] + h, v[1]:v[1] + w]
        _same(rows, ref, str(v))


def test_mixed_batch_keeps_plain_images_on_the_plain_kernel(ctx):
    pxs = [F.photo(70, 45, seed=s) for s in range(3)]
    plain = [F.jpeg(pxs[0], subsampling=2), F.jpeg(pxs[1][..., 0].copy()), F.jpeg(pxs[2], subsampling=0)]
    viewed = [_oriented(pxs[0], 6, subsampling=2), _oriented(pxs[1], 4, subsampling=1), _oriented(pxs[2], 7)]
    blobs = [plain[0], viewed[0], plain[1], viewed[1], viewed[2], plain[2]]
    views = [None, (6, 0, 0, 0, 0), None, (4, 3, 2, 33, 40), (7, 0, 0, 0, 0), None]
    ex = ctx.jpeg_decode_host(plain)
    got = ctx.jpeg_decode_host(blobs, views=views)
    for k, i in enumerate((0, 2, 5)):
        _same(got[i], ex[k], f"plain image {k} beside viewed ones")
    for i in (1, 3, 4):
        v = views[i]
        _same(got[i], F.reference(blobs[i], v[1:] if v[3] else None), f"viewed image {i}")


def test_view_kernel_is_timed_under_its_own_name(ctx):
    blob = _oriented(F.photo(97, 61), 6, subsampling=2)
    ctx.set_timing(True)
    try:
        ctx.reset_stats()
        ctx.jpeg_decode_host([blob, F.jpeg(F.photo(40, 30))], views=[(6, 0, 0, 0, 0), None])
        ms, n, _ = ctx.stats("k_jpeg_color_view")
        assert n >= 1 and ms > 0
        assert ctx.stats("k_jpeg_color")[1] >= 1
    finally:
        ctx.set_timing(False)


def test_view_batch_beyond_2_20_tiles(ctx):
    """520 1080p images at orientation 6 in one call: 2040 tiles each, so the
    1 060 800 work items exceed the 2^20-workgroup grid and the workgroups
    stride over them (the LDS tile reused behind a second barrier)."""
    W, H, N = 1920, 1080, 520
    assert N * ((W + 31) // 32) * ((H + 31) // 32) > 1 << 20
    blob = _oriented(F.photo(W, H), 6, subsampling=2, quality=90)
    ref = F.reference(blob)
    assert ref.shape == (W, H, 3)
    stride, size = H * 3, H * 3 * W
    base = ctx.malloc(size * N)
    try:
        st = ctx.jpeg_decode([blob] * N, [base + i * size for i in range(N)], [stride] * N, views=[(6, 0, 0, 0, 0)] * N)
        assert st == [0] * N
        for i in (0, 1, 513, 514, N - 1):  # (item 2^20 falls in image 514)
            assert np.array_equal(ctx.d2h(base + i * size, size).reshape(W, H, 3), ref), i
    finally:
        ctx.free(base)


def _pipeline_inputs():
    px = F.photo(320, 240, seed=3)
    blobs = [F.pillow_oriented(px, o, quality=90, subsampling=2) for o in range(2, 9)]
    opts = ["w_100", "w_120,h_90,c_1", "w_90,q_80", "w_100,smc_1", "w_80", "w_64,h_64,c_1", "w_111"]
    blobs.append(F.jpeg(px, quality=90, subsampling=2))  # e_1 on an unrotated source at an odd origin
    opts.append("e_1,p1x_33,p1y_17,p2x_250,p2y_200,w_100")
    blobs.append(F.pillow_oriented(px, 6, quality=90, subsampling=2))  # e_1 on an orientation-6 source (240 x 320)
    opts.append("e_1,p1x_21,p1y_35,p2x_400,p2y_300,w_90")
    blobs.append(F.jpeg(px, quality=85, subsampling=0))
    opts.append("w_150")
    blobs.append(F.splice(F.jpeg(px, quality=90), F.xmp_app1(6)))  # the XMP-only file: host
    opts.append("w_100")
    png = io.BytesIO()
    Image.fromarray(px).save(png, "PNG")
    blobs.append(png.getvalue())  # host
    opts.append("w_100,q_80")
    return blobs, opts


def test_pipeline_gpu_orient_matches_host_decode(ctx):
    blobs, opts = _pipeline_inputs()
    res, stats = {}, {}
    for name, kw in (("gpu", dict(gpu_orient=True)), ("host", dict(gpu_decode=False))):
        pipe = CodecPipeline(ctx, threads=4, **kw)
        try:
            res[name] = pipe.process(blobs, opts)
            stats[name] = dict(pipe.decode_stats)
        finally:
            pipe.close()
    (ea, ra), (eb, rb) = res["gpu"], res["host"]
    key = ("out_w", "out_h", "crop_x", "crop_y", "crop_w", "crop_h", "status")
    assert [[getattr(r, k) for k in key] for r in ra] == [[getattr(r, k) for k in key] for r in rb]
    for i, (a, b) in enumerate(zip(ea, eb)):
        assert a == b, f"image {i} ({opts[i]}): the encoded outputs differ"
    assert stats["gpu"] == {"gpu": len(blobs) - 2, "host": 2}
    assert stats["host"] == {"gpu": 0, "host": len(blobs)}
    assert ra[8].out_w == 90 and ra[7].out_w == 100  # (the extracts were resized from their rectangles)


def test_pipeline_extract_outside_the_oriented_image_raises_on_both_arms(ctx):
    px = F.photo(320, 240, seed=3)
    blob = F.pillow_oriented(px, 6, quality=90)  # oriented: 240 x 320
    opt = "e_1,p1x_250,p1y_10,p2x_300,p2y_100,w_50"  # inside 320 x 240, outside 240 x 320
    msgs = []
    for kw in (dict(gpu_orient=True), dict(gpu_decode=False)):
        pipe = CodecPipeline(ctx, threads=2, **kw)
        try:
            with pytest.raises(ExecFailedException) as e:
                pipe.process([blob], [opt])
            msgs.append(str(e.value))
        finally:
            pipe.close()
    assert msgs[0] == msgs[1] and "geometry does not contain image" in msgs[0]
