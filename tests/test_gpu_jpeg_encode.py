"""GPU JPEG encode (fi_jpeg_enc.hip) against libjpeg-turbo through Pillow
12.2.0: the whole file is byte-identical with Image.save(buf, "JPEG",
quality=q, subsampling=s, restart_marker_rows=1) for 4:4:4 / 4:2:0 / gray
images, tiny, odd and 8-mod-16 sizes (dummy blocks, the bottom chroma rule),
every quality regime, noise (0xFF stuffing, long codes), strided sources and
mixed batches; error statuses leave the rest of the batch intact, and
CodecPipeline(gpu_encode=True) writes the same pixels the host encoder does."""
import io

import numpy as np
import pytest
from PIL import Image

from flyimg_amd import _lib as L
from flyimg_amd.runtime import Context, jpeg_encode_bound
from flyimg_amd.synth import synth_rgb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _pillow(px, quality, subsampling=0):
    b = io.BytesIO()
    kw = dict(subsampling=subsampling) if px.ndim == 3 else {}
    Image.fromarray(px).save(b, "JPEG", quality=quality, restart_marker_rows=1, **kw)
    return b.getvalue()


def _same(got, ref, what):
    assert got is not None, what
    if got != ref:
        k = next((i for i in range(min(len(got), len(ref))) if got[i] != ref[i]), min(len(got), len(ref)))
        raise AssertionError(f"{what}: {len(got)} bytes against Pillow's {len(ref)}, first difference at byte {k}")


SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 23), (40, 56), (33, 65), (333, 211), (500, 281)]


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_jpeg_encode_byte_identical(ctx, w, h):
    px = synth_rgb(w, h, 11 + w + h)
    gray = np.ascontiguousarray(px[..., 1])
    got = ctx.jpeg_encode_host([px, px, gray], [90, 75, 80], [0, 2, 0])
    _same(got[0], _pillow(px, 90, 0), f"{w}x{h} 4:4:4 q90")
    _same(got[1], _pillow(px, 75, 2), f"{w}x{h} 4:2:0 q75")
    _same(got[2], _pillow(gray, 80), f"{w}x{h} gray q80")


@pytest.mark.parametrize("q", [1, 30, 50, 89, 90, 100])
def test_jpeg_encode_qualities(ctx, q):
    px = synth_rgb(97, 61, 5)
    got = ctx.jpeg_encode_host([px, px], q, [0, 2])
    _same(got[0], _pillow(px, q, 0), f"q{q} 4:4:4")
    _same(got[1], _pillow(px, q, 2), f"q{q} 4:2:0")


@pytest.mark.parametrize("ss", [0, 2])
def test_jpeg_encode_noise(ctx, ss):
    """Uniform noise at q100: 0xFF stuffing, the longest codes, and the bound."""
    px = np.random.default_rng(ss).integers(0, 256, (157, 211, 3), dtype=np.uint8)
    got = ctx.jpeg_encode_host([px], 100, ss)[0]
    _same(got, _pillow(px, 100, ss), f"noise ss{ss}")
    assert b"\xff\x00" in got
    assert len(got) <= jpeg_encode_bound(211, 157, 3, 100, ss)


def test_jpeg_encode_strided_view(ctx):
    """A sub-rectangle of a larger device image: pointer offset, stride larger
    than the width, a start that is not 16-byte aligned."""
    big = synth_rgb(300, 200, 21)
    p = ctx.malloc(big.nbytes)
    try:
        ctx.h2d(p, big)
        x0, y0, w, h = 27, 13, 181, 95
        view = (p + y0 * 900 + x0 * 3, w, h, 900, 3)
        assert view[0] % 16 != 0
        got = ctx.jpeg_encode([view, view], [90, 60], [0, 2])
    finally:
        ctx.free(p)
    sl = np.ascontiguousarray(big[y0:y0 + h, x0:x0 + w])
    _same(got[0], _pillow(sl, 90, 0), "strided 4:4:4")
    _same(got[1], _pillow(sl, 60, 2), "strided 4:2:0")


def test_jpeg_encode_mixed_batch_with_rejected_images(ctx):
    """One call: sizes, channel counts, qualities and subsamplings mixed; an
    RGBA image is FI_EUNSUPPORTED, quality 0 and a 4:2:2 request fail with
    their statuses, the others are byte-identical."""
    rgb = [synth_rgb(w, h, 30 + i) for i, (w, h) in enumerate(
        [(120, 80), (31, 45), (64, 64), (200, 8), (8, 200), (77, 55), (130, 129), (24, 40)])]
    images = rgb + [np.ascontiguousarray(rgb[0][..., 0]), np.ascontiguousarray(rgb[5][..., 2]),
                    np.dstack([rgb[1], rgb[1][..., :1]]), rgb[2], rgb[3]]
    quality = [90, 75, 100, 30, 85, 50, 95, 10, 80, 60, 90, 0, 90]
    sub = [0, 2, 2, 0, 2, 0, 2, 2, 0, 2, 0, 0, 1]
    ptrs = [ctx.malloc(a.nbytes) for a in images]
    try:
        views = []
        for a, p in zip(images, ptrs):
            ctx.h2d(p, a)
            c = a.shape[2] if a.ndim == 3 else 1
            views.append((p, a.shape[1], a.shape[0], a.shape[1] * c, c))
        rc, status, lens, bufs = ctx.jpeg_encode_raw(views, quality, sub)
    finally:
        for p in ptrs:
            ctx.free(p)
    assert status[10] == L.FI_EUNSUPPORTED and status[11] == L.FI_EINVAL and status[12] == L.FI_EUNSUPPORTED
    assert rc == L.FI_EUNSUPPORTED  # the first failing status
    for i in range(10):
        assert status[i] == L.FI_OK, i
        _same(bufs[i][:lens[i]].tobytes(), _pillow(images[i], quality[i], sub[i]), f"image {i}")


def test_jpeg_encode_capacity(ctx):
    """out_cap one byte short: the out-of-memory status with the true length,
    nothing written past out_cap, the neighbour encoded."""
    a, b = synth_rgb(90, 70, 1), synth_rgb(50, 60, 2)
    ref_a, ref_b = _pillow(a, 85, 2), _pillow(b, 85, 2)
    ptrs = [ctx.malloc(x.nbytes) for x in (a, b)]
    try:
        ctx.h2d(ptrs[0], a)
        ctx.h2d(ptrs[1], b)
        views = [(ptrs[0], 90, 70, 270, 3), (ptrs[1], 50, 60, 150, 3)]
        cap = len(ref_a) - 1
        rc, status, lens, bufs = ctx.jpeg_encode_raw(views, 85, 2, caps=[cap, len(ref_b)])
    finally:
        for p in ptrs:
            ctx.free(p)
    assert rc == L.FI_ENOMEM and status == [L.FI_ENOMEM, L.FI_OK]
    assert lens == [len(ref_a), len(ref_b)]
    assert bufs[0].size == cap + 64 and np.all(bufs[0][cap:] == 0xA5)  # the guard bytes behind out_cap
    assert bufs[1][:lens[1]].tobytes() == ref_b and np.all(bufs[1][lens[1]:] == 0xA5)


def test_jpeg_encode_round_trip_through_gpu_decoder(ctx):
    """The GPU decoder reads the encoder's files as Pillow does: 640x481 at
    4:2:0 (31 restart intervals), a 4:4:4 and a gray one."""
    px = synth_rgb(640, 481, 8)
    files = ctx.jpeg_encode_host([px, synth_rgb(123, 77, 9), np.ascontiguousarray(px[:100, :90, 0])],
                                 [75, 92, 70], [2, 0, 0])
    assert files[0].count(b"\xff\xd0") >= 3  # RST0 .. RST7 cycle over the rows
    back = ctx.jpeg_decode_host(files)
    for f, got in zip(files, back):
        ref = np.asarray(Image.open(io.BytesIO(f)))
        assert got is not None and got.shape == ref.shape and np.array_equal(got, ref)


def test_jpeg_encode_widest_image(ctx):
    """65500 pixels wide (libjpeg's own limit, so Pillow can write the
    reference): 8188 blocks in one restart interval, 128 passes of the entropy
    coder with the partial byte carried between them."""
    px = np.ascontiguousarray(synth_rgb(65500, 3, 4)[..., 0])
    _same(ctx.jpeg_encode_host([px], 50, 0)[0], _pillow(px, 50), "65500x3 gray")


def test_jpeg_encode_scratch_beyond_2_31_bytes(ctx):
    """56 1080p 4:4:4 images in one call: their worst-case interval slots span
    2.26 GB, so slot and block offsets past 2^31 are exercised (one shared
    source image; every file must be the same bytes)."""
    W, H, N = 1920, 1080, 56
    px = synth_rgb(W, H, 17)
    ref = _pillow(px, 90, 0)
    p = ctx.malloc(px.nbytes)
    try:
        ctx.h2d(p, px)
        files = ctx.jpeg_encode([(p, W, H, W * 3, 3)] * N, 90, 0)
    finally:
        ctx.free(p)
    assert N * 135 * (720 * 416 + 2) > 2 ** 31
    for i in (0, 27, 53, N - 1):
        _same(files[i], ref, f"image {i}")
    assert all(len(f) == len(ref) for f in files)


def test_jpeg_encode_kernel_stats(ctx):
    ctx.set_timing(1)
    ctx.reset_stats()
    try:
        ctx.jpeg_encode_host([synth_rgb(64, 48, 1)], 90, 0)
        for name in ("k_jpeg_fdct", "k_jpeg_henc", "k_jpeg_pack"):
            ms, launches, _ = ctx.stats(name)
            assert launches == 1 and ms > 0, name
    finally:
        ctx.set_timing(0)
        ctx.reset_stats()


def test_codec_pipeline_gpu_encode(ctx):
    """CodecPipeline(gpu_encode=True) on the mixed batch of
    test_codec_pipeline_gpu_decode_equals_host_decode plus an RGBA PNG: same
    records; every JPEG is Pillow's restart_marker_rows=1 file of the pixels
    the host-encode pipeline wrote; both pipelines' outputs decode to the same
    arrays; the PNG output is unchanged."""
    from flyimg_amd.codec import CodecPipeline, decode

    def enc(img, **kw):
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", **kw)
        return b.getvalue()

    rot = io.BytesIO()
    im = Image.fromarray(synth_rgb(300, 200, 9))
    ex = im.getexif()
    ex[0x0112] = 6
    im.save(rot, "JPEG", quality=90, exif=ex.tobytes())
    png = io.BytesIO()
    Image.fromarray(synth_rgb(320, 240, 10)).save(png, "PNG")
    rgba = io.BytesIO()
    Image.fromarray(np.dstack([synth_rgb(200, 150, 12), synth_rgb(200, 150, 13)[..., :1]])).save(rgba, "PNG")
    blobs = [
        enc(synth_rgb(1280, 720, 1), quality=90, subsampling=2),
        enc(synth_rgb(999, 555, 2), quality=85, subsampling=0),
        enc(synth_rgb(800, 600, 3), quality=90, subsampling=2),
        enc(synth_rgb(640, 480, 4), quality=90, progressive=True),
        rot.getvalue(),
        png.getvalue(),
        enc(synth_rgb(720, 480, 11)[..., 1].copy(), quality=90),
        rgba.getvalue(),
    ]
    opts = ["w_500,smc_1,q_90", "w_300,h_250,c_1", "e_1,p1x_100,p1y_50,p2x_700,p2y_450,w_200",
            "w_200,h_200,c_1", "w_150", "w_100,q_80", "w_300,h_200,c_1", "w_120"]
    quality = [90, 90, 90, 90, 90, 80, 90, 90]
    res = {}
    for ge in (True, False):
        pipe = CodecPipeline(ctx, threads=4, gpu_encode=ge)
        try:
            res[ge] = pipe.process(blobs, opts)
        finally:
            pipe.close()
    (ea, ra), (eb, rb) = res[True], res[False]
    key = ("out_w", "out_h", "out_channels", "crop_x", "crop_y", "crop_w", "crop_h", "status")
    assert [[getattr(r, k) for k in key] for r in ra] == [[getattr(r, k) for k in key] for r in rb]
    assert ea[7] == eb[7] and eb[7][:4] == b"\x89PNG"
    for i in range(7):
        assert eb[i][:2] == b"\xff\xd8"
        assert np.array_equal(decode(ea[i]), decode(eb[i])), i  # same coefficients, same pixels
    # the pixels the host-encode pipeline handed to its encoder: the same run
    # once more with codec.encode watched (its files are eb again)
    import flyimg_amd.codec as codec

    kept, orig = {}, codec.encode

    def spy(px, q=90):
        f = orig(px, q)
        kept[f] = np.array(px)
        return f

    pipe = CodecPipeline(ctx, threads=4)
    codec.encode = spy
    try:
        ec, _ = pipe.process(blobs, opts)
    finally:
        codec.encode = orig
        pipe.close()
    assert ec == eb
    for i in range(7):
        _same(ea[i], _pillow(kept[eb[i]], quality[i], 0 if quality[i] >= 90 else 2), f"pipeline output {i}")


def test_jpeg_encode_scan_chunk_carry(ctx):
    """One call whose restart intervals cross the 256-item chunks of the
    batch's scan (enc_scan_items): gray images of 254, 3 and 300 MCU rows, so
    the second image's intervals are items 254..256 -- its start is written in
    the first chunk, its end in the second, from the carried total -- and the
    third image's run across the second boundary to item 556."""
    images = [np.ascontiguousarray(synth_rgb(8, h, 70 + h)[..., 1]) for h in (2032, 24, 2400)]
    assert [(-(-a.shape[0] // 8), a.shape[1]) for a in images] == [(254, 8), (3, 8), (300, 8)]
    got = ctx.jpeg_encode_host(images, [90, 75, 85], 0)
    for k, (a, q) in enumerate(zip(images, [90, 75, 85])):
        _same(got[k], _pillow(a, q), f"image {k}: 8x{a.shape[0]} gray q{q}")
