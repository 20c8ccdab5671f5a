"""Progressive GPU JPEG encode (fi_jpeg_penc.hip, FI_JPEG_ENC_PROGRESSIVE)
against libjpeg-turbo through Pillow: the whole file is byte-identical with
Image.save(buf, "JPEG", quality=q, subsampling=s, progressive=True,
restart_marker_rows=1) -- ten scans (six for gray) with Huffman tables fitted
to each -- over the sizes, qualities and noise of the baseline encoder's tests,
the image that overflows the correction-bit buffer inside EOB runs, strided
sources and mixed batches with rejected images; flags 0 is the baseline
encoder; the library's own progressive decoder reads the files; and
CodecPipeline(gpu_encode=True, gpu_progressive_encode=True) writes them."""
import io

import numpy as np
import pytest
from PIL import Image

from flyimg_amd import _lib as L
from flyimg_amd.runtime import Context, jpeg_encode_bound
from flyimg_amd.synth import synth_rgb

from .test_jpeg_penc_cpu import QUALITIES, SIZES, flush_image, pillow_progressive as _pillow, same as _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_progressive_encode_byte_identical(ctx, w, h):
    px = synth_rgb(w, h, 11 + w + h)
    gray = np.ascontiguousarray(px[..., 1])
    got = ctx.jpeg_encode_host([px, px, gray], [90, 75, 80], [0, 2, 0], progressive=True)
    _same(got[0], _pillow(px, 90, 0), f"{w}x{h} 4:4:4 q90")
    _same(got[1], _pillow(px, 75, 2), f"{w}x{h} 4:2:0 q75")
    _same(got[2], _pillow(gray, 80), f"{w}x{h} gray q80")


@pytest.mark.parametrize("q", QUALITIES)
def test_progressive_encode_qualities(ctx, q):
    px = synth_rgb(97, 61, 5)
    got = ctx.jpeg_encode_host([px, px], q, [0, 2], progressive=True)
    _same(got[0], _pillow(px, q, 0), f"q{q} 4:4:4")
    _same(got[1], _pillow(px, q, 2), f"q{q} 4:2:0")


@pytest.mark.parametrize("ss", [0, 2])
def test_progressive_encode_noise(ctx, ss):
    """Uniform noise at q100: 0xFF stuffing, long codes, and the bound."""
    px = np.random.default_rng(ss).integers(0, 256, (157, 211, 3), dtype=np.uint8)
    got = ctx.jpeg_encode_host([px], 100, ss, progressive=True)[0]
    _same(got, _pillow(px, 100, ss), f"noise ss{ss}")
    assert b"\xff\x00" in got
    assert len(got) <= jpeg_encode_bound(211, 157, 3, 100, ss, progressive=True)


def test_progressive_encode_flush_image(ctx):
    """Every block row of the last scan is one EOB run whose correction bits
    pass 937 several times (test_jpeg_penc_cpu counts the flushes in the model)."""
    px = flush_image()
    _same(ctx.jpeg_encode_host([px], 100, 0, progressive=True)[0], _pillow(px, 100), "flush image")


def test_progressive_encode_strided_view(ctx):
    """A sub-rectangle of a larger device image: pointer offset, stride larger
    than the width, a start that is not 16-byte aligned."""
    big = synth_rgb(300, 200, 21)
    p = ctx.malloc(big.nbytes)
    try:
        ctx.h2d(p, big)
        x0, y0, w, h = 27, 13, 181, 95
        view = (p + y0 * 900 + x0 * 3, w, h, 900, 3)
        assert view[0] % 16 != 0
        got = ctx.jpeg_encode([view, view], [90, 60], [0, 2], progressive=True)
    finally:
        ctx.free(p)
    sl = np.ascontiguousarray(big[y0:y0 + h, x0:x0 + w])
    _same(got[0], _pillow(sl, 90, 0), "strided 4:4:4")
    _same(got[1], _pillow(sl, 60, 2), "strided 4:2:0")


def _upload(ctx, images):
    ptrs = [ctx.malloc(a.nbytes) for a in images]
    views = []
    for a, p in zip(images, ptrs):
        ctx.h2d(p, a)
        c = a.shape[2] if a.ndim == 3 else 1
        views.append((p, a.shape[1], a.shape[0], a.shape[1] * c, c))
    return ptrs, views


def test_progressive_encode_mixed_batch_with_rejected_images(ctx):
    """One call: sizes, channel counts, qualities and subsamplings mixed; an
    RGBA image is FI_EUNSUPPORTED, quality 0 and a 4:2:2 request fail with
    their statuses, the others are byte-identical."""
    rgb = [synth_rgb(w, h, 30 + i) for i, (w, h) in enumerate(
        [(120, 80), (31, 45), (64, 64), (200, 8), (8, 200), (77, 55), (130, 129), (24, 40)])]
    images = rgb + [np.ascontiguousarray(rgb[0][..., 0]), np.ascontiguousarray(rgb[5][..., 2]),
                    np.dstack([rgb[1], rgb[1][..., :1]]), rgb[2], rgb[3]]
    quality = [90, 75, 100, 30, 85, 50, 95, 10, 80, 60, 90, 0, 90]
    sub = [0, 2, 2, 0, 2, 0, 2, 2, 0, 2, 0, 0, 1]
    ptrs, views = _upload(ctx, images)
    try:
        rc, status, lens, bufs = ctx.jpeg_encode_raw(views, quality, sub, progressive=True)
    finally:
        for p in ptrs:
            ctx.free(p)
    assert status[10] == L.FI_EUNSUPPORTED and status[11] == L.FI_EINVAL and status[12] == L.FI_EUNSUPPORTED
    assert rc == L.FI_EUNSUPPORTED  # the first failing status
    for i in range(10):
        assert status[i] == L.FI_OK, i
        _same(bufs[i][:lens[i]].tobytes(), _pillow(images[i], quality[i], sub[i]), f"image {i}")


def test_encode_ex_with_flags_0_is_the_baseline_encoder(ctx):
    images = [synth_rgb(90, 70, 1), np.ascontiguousarray(synth_rgb(50, 60, 2)[..., 0])]
    ptrs, views = _upload(ctx, images)
    try:
        rc0, st0, len0, buf0 = ctx.jpeg_encode_raw(views, [85, 90], [2, 0])
        n = len(views)
        I32, I64, SZ, VP = L.ctypes.c_int32 * n, L.ctypes.c_int64 * n, L.ctypes.c_size_t * n, L.ctypes.c_void_p * n
        caps = [jpeg_encode_bound(v[1], v[2], v[4], q, s) for v, q, s in zip(views, [85, 90], [2, 0])]
        outs = [np.empty(c, np.uint8) for c in caps]
        out_len, status = SZ(), I32()
        rc = L.lib().fi_jpeg_encode_device_ex(
            ctx.h, VP(*[v[0] for v in views]), I32(*[v[1] for v in views]), I32(*[v[2] for v in views]),
            I32(*[v[4] for v in views]), I64(*[v[3] for v in views]), I32(85, 90), I32(2, 0), n,
            VP(*[o.ctypes.data for o in outs]), SZ(*caps), out_len, status, 0)
        bad = L.lib().fi_jpeg_encode_device_ex(
            ctx.h, VP(*[v[0] for v in views]), I32(*[v[1] for v in views]), I32(*[v[2] for v in views]),
            I32(*[v[4] for v in views]), I64(*[v[3] for v in views]), I32(85, 90), I32(2, 0), n,
            VP(*[o.ctypes.data for o in outs]), SZ(*caps), out_len, status, 2)
    finally:
        for p in ptrs:
            ctx.free(p)
    assert rc0 == L.FI_OK and rc == L.FI_OK and list(status) == [0, 0] and bad == L.FI_EINVAL
    for i in range(n):
        assert outs[i][:out_len[i]].tobytes() == buf0[i][:len0[i]].tobytes()
        assert outs[i][:2].tobytes() == b"\xff\xd8" and b"\xff\xc0" in outs[i][:700].tobytes()


def test_progressive_encode_capacity(ctx):
    """out_cap one byte short: the out-of-memory status with the true length,
    nothing written past out_cap, the neighbour encoded."""
    a, b = synth_rgb(90, 70, 1), synth_rgb(50, 60, 2)
    ref_a, ref_b = _pillow(a, 85, 2), _pillow(b, 85, 2)
    ptrs, views = _upload(ctx, [a, b])
    try:
        cap = len(ref_a) - 1
        rc, status, lens, bufs = ctx.jpeg_encode_raw(views, 85, 2, caps=[cap, len(ref_b)], progressive=True)
    finally:
        for p in ptrs:
            ctx.free(p)
    assert rc == L.FI_ENOMEM and status == [L.FI_ENOMEM, L.FI_OK]
    assert lens == [len(ref_a), len(ref_b)]
    assert bufs[0].size == cap + 64 and np.all(bufs[0][cap:] == 0xA5)  # the guard bytes behind out_cap
    assert bufs[1][:lens[1]].tobytes() == ref_b and np.all(bufs[1][lens[1]:] == 0xA5)


def test_progressive_encode_round_trip_through_gpu_decoder(ctx):
    """The library's progressive decoder reads the encoder's files as Pillow
    does: 4:2:0 (more than 8 block rows: the RSTn cycle), 4:4:4 and gray."""
    px = synth_rgb(320, 241, 8)
    files = ctx.jpeg_encode_host([px, synth_rgb(123, 77, 9), np.ascontiguousarray(px[:100, :90, 0])],
                                 [75, 92, 70], [2, 0, 0], progressive=True)
    assert all(f is not None and b"\xff\xc2" in f[:700] for f in files)
    back = ctx.jpeg_decode_host(files, progressive=True)
    for f, got in zip(files, back):
        ref = np.asarray(Image.open(io.BytesIO(f)))
        assert got is not None and got.shape == ref.shape and np.array_equal(got, ref)


def test_progressive_encode_kernel_stats(ctx):
    ctx.set_timing(1)
    ctx.reset_stats()
    try:
        ctx.jpeg_encode_host([synth_rgb(64, 48, 1)], 90, 0, progressive=True)
        for name in ("k_jpeg_fdct", "k_jpeg_pstat", "k_jpeg_ptab", "k_jpeg_pcode", "k_jpeg_ppack"):
            ms, launches, _ = ctx.stats(name)
            assert launches == 1 and ms > 0, name
    finally:
        ctx.set_timing(0)
        ctx.reset_stats()


def _sof(blob):
    """The marker of the file's frame header."""
    i = 2
    while True:
        assert blob[i] == 0xFF
        if 0xC0 <= blob[i + 1] <= 0xCF and blob[i + 1] not in (0xC4, 0xC8, 0xCC):
            return blob[i + 1]
        i += 2 + (blob[i + 2] << 8 | blob[i + 3])


def test_codec_pipeline_gpu_progressive_encode(ctx):
    """CodecPipeline(gpu_encode=True, gpu_progressive_encode=True) on a small
    mixed batch: the RGBA output is still a PNG; every JPEG output has an SOF2
    frame, decodes to the pixels of the baseline gpu_encode output, and is
    Pillow's progressive file of those pixels."""
    from flyimg_amd.codec import CodecPipeline, decode

    def enc(img, fmt="JPEG", **kw):
        b = io.BytesIO()
        Image.fromarray(img).save(b, fmt, **kw)
        return b.getvalue()

    with pytest.raises(ValueError):
        CodecPipeline(ctx, threads=1, gpu_progressive_encode=True)
    blobs = [enc(synth_rgb(640, 360, 1), quality=90, subsampling=2),
             enc(synth_rgb(333, 255, 2), quality=85, subsampling=0),
             enc(synth_rgb(360, 240, 11)[..., 1].copy(), quality=90),
             enc(np.dstack([synth_rgb(200, 150, 12), synth_rgb(200, 150, 13)[..., :1]]), "PNG")]
    opts = ["w_250,smc_1,q_90", "w_150,h_120,c_1,q_80", "w_200,h_100,c_1", "w_120"]
    quality = [90, 80, 90, 90]
    res = {}
    for prog in (True, False):
        pipe = CodecPipeline(ctx, threads=4, gpu_encode=True, gpu_progressive_encode=prog)
        try:
            res[prog] = pipe.process(blobs, opts)[0]
        finally:
            pipe.close()
    ea, eb = res[True], res[False]
    assert ea[3] == eb[3] and ea[3][:4] == b"\x89PNG"
    for i in range(3):
        assert _sof(ea[i]) == 0xC2 and _sof(eb[i]) == 0xC0
        px = decode(eb[i])
        assert np.array_equal(decode(ea[i]), px), i
    ref = _reference_files(ctx, blobs, opts, quality)
    for i in range(3):
        _same(ea[i], ref[i], f"pipeline output {i}")


def _reference_files(ctx, blobs, opts, quality):
    """Pillow's progressive files of the pixels the host-encode pipeline hands
    to its encoder (codec.encode watched, as test_gpu_jpeg_encode does)."""
    import flyimg_amd.codec as codec
    from flyimg_amd.codec import CodecPipeline

    kept, orig = [], codec.encode

    def spy(px, q=90):
        f = orig(px, q)
        kept.append((f, np.array(px)))
        return f

    pipe = CodecPipeline(ctx, threads=4)
    codec.encode = spy
    try:
        files, _ = pipe.process(blobs, opts)
    finally:
        codec.encode = orig
        pipe.close()
    by_file = {f: px for f, px in kept}
    return [_pillow(by_file[files[i]], quality[i], 0 if quality[i] >= 90 else 2)
            for i in range(len(blobs)) if files[i][:2] == b"\xff\xd8"]


def _pieces(blob):
    """The pieces jpeg_pencode_batch packs for this file: the head, per scan
    its DHT segments, its DRI / SOS bytes and its restart intervals, EOI."""
    ndht = nsos = nrst = 0
    i = 2
    while i < len(blob):
        assert blob[i] == 0xFF
        m = blob[i + 1]
        if m == 0xD9:
            break
        ndht += m == 0xC4
        i += 2 + int.from_bytes(blob[i + 2:i + 4], "big")
        if m == 0xDA:  # entropy-coded data up to the next marker that is no RSTn
            nsos += 1
            while not (blob[i] == 0xFF and blob[i + 1] != 0 and not 0xD0 <= blob[i + 1] <= 0xD7):
                nrst += blob[i] == 0xFF and 0xD0 <= blob[i + 1] <= 0xD7
                i += 1
    return 1 + ndht + nsos + (nrst + nsos) + 1


def test_progressive_encode_pieces_cross_the_scan_chunk(ctx):
    """One call whose pieces cross the 256-item chunk of the batch's scan
    (enc_scan_items): 24 x 24 RGB 4:2:0 images have some 45 pieces each (10
    scans; three images stay below 256), so eight of them."""
    images = [synth_rgb(24, 24, 90 + k) for k in range(8)]
    quality = [90, 75, 50, 95, 85, 60, 30, 100]
    refs = [_pillow(a, q, 2) for a, q in zip(images, quality)]
    npieces = [_pieces(r) for r in refs]
    assert sum(npieces[:3]) < 256 < sum(npieces), npieces
    got = ctx.jpeg_encode_host(images, quality, 2, progressive=True)
    for k in range(8):
        _same(got[k], refs[k], f"image {k} q{quality[k]}")
