"""GPU lossless WebP encode (fi_webp_enc.hip).  The host form
fi_debug_webp_encode_host runs the same inline code on the CPU and is the
specification: every device file must equal it byte for byte, and Pillow
(libwebp) must return the input pixels.  On top: forced predictors, strided
views, mixed batches with rejected images, the capacity rule, the kernel
statistics, the size against the GPU PNG encoder and the pipeline switch.  Crafted content
-- codes the 15-bit limit shapes, literals above 48 bits, the length and
distance ladders, band edges -- is in tests/_lossless_content.py,
tests/test_lossless_content_cpu.py and tests/test_gpu_lossless_content.py."""
import io
import os

import numpy as np
import pytest
from PIL import Image

from flyimg_amd import _lib as L
from flyimg_amd.runtime import Context, webp_encode_bound, webp_encode_host_form
from flyimg_amd.synth import synth_rgb

from .test_webp_encode_cpu import channels, check_file, content, table_inputs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _check(ctx, images, predictor=-1, literal=False):
    """One device call: every file equals the host form and decodes to its source."""
    files = ctx.webp_encode_host(images, predictor)
    preds = list(predictor) if isinstance(predictor, (list, tuple)) else [predictor] * len(images)
    for px, f, p in zip(images, files, preds):
        px3 = px if px.ndim == 3 else px[..., None]
        assert f is not None
        assert len(f) <= webp_encode_bound(px3.shape[1], px3.shape[0], px3.shape[2])
        assert f == webp_encode_host_form(px3, p), (px3.shape, p)
        check_file(f, px3, literal=literal)
    return files


@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (7, 1), (3, 5), (16, 17), (17, 16), (63, 2), (65, 2)])
def test_webp_encode_small_geometries(ctx, w, h):
    _check(ctx, [channels(content("synth", w, h), c) for c in (1, 2, 3, 4)], literal=True)


@pytest.mark.parametrize("w,h,chans", [(90, 91, (4,)), (91, 91, (4,)), (200, 200, (4, 2)), (333, 211, (3, 1))])
def test_webp_encode_bands(ctx, w, h, chans):
    """8190 pixels are one band, 8281 two; the larger images have 5 and 9."""
    _check(ctx, [channels(content("synth", w, h), c) for c in chans])


def test_webp_encode_every_predictor(ctx):
    px = content("gradient", 37, 53)
    files = _check(ctx, [px] * 15, list(range(14)) + [-1])
    assert len(set(files)) > 10  # the modes act


def test_webp_encode_flat_and_checkerboard(ctx):
    images = [channels(content(name, w, h), c) for name in ("flat", "checker") for (w, h) in ((200, 200), (97, 61))
              for c in (1, 4)]
    files = _check(ctx, images)
    assert all(len(f) < 100 for f in files[:4])  # flat: a literal and a few copies per band


def test_webp_encode_noise_stays_within_the_bound(ctx):
    images = [channels(content("noise", 150, 77), c) for c in (1, 2, 3, 4)]
    files = _check(ctx, images)  # (checks len(f) <= webp_encode_bound)
    for f, px in zip(files, images):
        assert len(f) >= px.size  # nothing to gain: the fallback form


def test_webp_encode_tiled_pattern_and_batch_of_contents(ctx):
    _check(ctx, [channels(content(name, 97, 61), c) for name in ("tiled", "gradient", "synth") for c in (2, 3)])


def test_webp_encode_strided_view(ctx):
    """A sub-rectangle of a larger device image whose surroundings are poison:
    pointer offset, stride larger than the width, unaligned starts."""
    big = channels(content("synth", 300, 200), 4)
    poison = np.full_like(big, 0xEE)
    x0, y0, w, h = 27, 13, 181, 95
    poison[y0:y0 + h, x0:x0 + w] = big[y0:y0 + h, x0:x0 + w]
    flat = poison.reshape(200, 1200)
    p = ctx.malloc(poison.nbytes)
    try:
        ctx.h2d(p, poison)
        view = (p + y0 * 1200 + x0 * 4, w, h, 1200, 4)
        odd = (p + y0 * 1200 + x0 * 4 + 1, 33, 40, 1200, 1)  # a gray view starting on an odd byte
        assert view[0] % 16 != 0 and odd[0] % 2 == 1
        got = ctx.webp_encode([view, odd, view], [-1, -1, 11])
    finally:
        ctx.free(p)
    sl = np.ascontiguousarray(big[y0:y0 + h, x0:x0 + w])
    sl1 = np.ascontiguousarray(flat[y0:y0 + 40, x0 * 4 + 1:x0 * 4 + 1 + 33])[..., None]
    assert got[0] == webp_encode_host_form(sl) and got[2] == webp_encode_host_form(sl, 11)
    assert got[1] == webp_encode_host_form(sl1)
    check_file(got[0], sl, literal=False)
    check_file(got[1], sl1, literal=False)
    check_file(got[2], sl, literal=False)


def _upload(ctx, images):
    ptrs = [ctx.malloc(a.nbytes) for a in images]
    views = []
    for a, p in zip(images, ptrs):
        ctx.h2d(p, a)
        views.append((p, a.shape[1], a.shape[0], a.shape[1] * a.shape[2], a.shape[2]))
    return ptrs, views


def test_webp_encode_mixed_batch_with_rejected_images(ctx):
    """One call: sizes, channel counts and predictors mixed; 5 channels and
    predictor 14 get FI_EINVAL, width 16385 FI_EUNSUPPORTED, the return code is
    the first failing status, the other files are intact."""
    sizes = [(120, 80), (31, 45), (64, 64), (200, 8), (8, 200), (77, 55), (130, 129), (24, 40)]
    images = [channels(content("synth", w, h, i), 1 + i % 4) for i, (w, h) in enumerate(sizes)]
    preds = [-1, 0, 5, 11, 12, 13, -1, -1]
    ptrs, views = _upload(ctx, images)
    try:
        bad = [(ptrs[0], 10, 10, 50, 5), (ptrs[0], 16385, 1, 16385 * 4, 4), (ptrs[0], 10, 10, 40, 4)]
        order = views[:3] + bad[:1] + views[3:6] + bad[1:] + views[6:]
        pl = preds[:3] + [-1] + preds[3:6] + [-1, 14] + preds[6:]
        rc, status, lens, bufs = ctx.webp_encode_raw(order, pl)
    finally:
        for p in ptrs:
            ctx.free(p)
    assert rc == L.FI_EINVAL
    assert [status[i] for i in (3, 7, 8)] == [L.FI_EINVAL, L.FI_EUNSUPPORTED, L.FI_EINVAL]
    assert [lens[i] for i in (3, 7, 8)] == [0, 0, 0]
    for k, i in enumerate([0, 1, 2, 4, 5, 6, 9, 10]):
        assert status[i] == L.FI_OK, i
        f = bufs[i][:lens[i]].tobytes()
        assert f == webp_encode_host_form(images[k], preds[k]), k
        check_file(f, images[k], literal=False)
        assert np.all(bufs[i][lens[i]:][-64:] == 0xA5)


def test_webp_encode_null_predictor_is_adaptive(ctx):
    px = content("synth", 70, 50)
    ptrs, views = _upload(ctx, [px])
    try:
        rc, status, lens, bufs = ctx.webp_encode_raw(views, None)
    finally:
        ctx.free(ptrs[0])
    assert rc == L.FI_OK and status == [L.FI_OK]
    assert bufs[0][:lens[0]].tobytes() == webp_encode_host_form(px, -1)


def test_webp_encode_capacity(ctx):
    """out_cap one byte short: FI_ENOMEM with the true length, the guard bytes
    behind the capacity untouched, the neighbour encoded; a second call with
    the reported size succeeds."""
    a, b = content("synth", 90, 70, 1), channels(content("synth", 50, 60, 2), 2)
    ptrs, views = _upload(ctx, [a, b])
    try:
        rc, status, lens, bufs = ctx.webp_encode_raw(views)
        assert rc == L.FI_OK
        ref_a, ref_b = bufs[0][:lens[0]].tobytes(), bufs[1][:lens[1]].tobytes()
        cap = len(ref_a) - 1
        rc, status, lens, bufs = ctx.webp_encode_raw(views, caps=[cap, len(ref_b)])
        assert rc == L.FI_ENOMEM and status == [L.FI_ENOMEM, L.FI_OK]
        assert lens == [len(ref_a), len(ref_b)]
        assert bufs[0].size == cap + 64 and np.all(bufs[0][cap:] == 0xA5)  # the guard bytes behind out_cap
        assert bufs[1][:lens[1]].tobytes() == ref_b and np.all(bufs[1][lens[1]:] == 0xA5)
        rc, status, lens, bufs = ctx.webp_encode_raw(views[:1], caps=[lens[0]])
        assert rc == L.FI_OK and status == [L.FI_OK] and bufs[0][:lens[0]].tobytes() == ref_a
    finally:
        for p in ptrs:
            ctx.free(p)
    assert ref_a == webp_encode_host_form(a) and ref_b == webp_encode_host_form(b)


def test_webp_encode_kernel_stats(ctx):
    ctx.set_timing(1)
    ctx.reset_stats()
    try:
        ctx.webp_encode_host([content("synth", 64, 48)])
        for name in ("k_webp_pred", "k_webp_lz", "k_webp_codes", "k_webp_emit", "k_webp_pack"):
            ms, launches, _ = ctx.stats(name)
            assert launches == 1 and ms > 0, name
    finally:
        ctx.set_timing(0)
        ctx.reset_stats()


def test_webp_files_are_no_larger_than_the_gpu_png_files(ctx):
    t = table_inputs()
    webp = _check(ctx, list(t.values()))
    png = ctx.png_encode_host(list(t.values()))
    for name, fw, fp in zip(t, webp, png):
        print(name, len(fw), len(fp))
        assert len(fw) <= len(fp), name


def test_codec_pipeline_gpu_webp(ctx):
    """o_webp,webpl_1 outputs leave as RIFF/WEBP files of exactly the pixels
    the pipeline holds on the device: what its PNG output decodes to without
    the switch, and for the opaque output what the batch computes before JPEG
    coding.  A bag without o_webp in the same batch still yields PNG or JPEG."""
    from flyimg_amd.codec import CodecPipeline, decode, decode_ex
    from flyimg_amd.processor import ImageProcessor, OptionsBag

    with open(os.path.join(GOLDEN, "square-opaque-200.png"), "rb") as f:
        square = f.read()
    b = io.BytesIO()
    Image.fromarray(synth_rgb(160, 120, 60)).save(b, "JPEG", quality=90)
    blobs = [square, b.getvalue(), square, b.getvalue()]
    opts = ["w_100,o_webp,webpl_1"] * 2 + ["w_100", "w_100,o_webp"]  # (webpl defaults to 0: not lossless, not ours)
    res = {}
    for name, kw in (("webp", dict(gpu_webp=True)), ("plain", {})):
        pipe = CodecPipeline(ctx, threads=4, gpu_encode=True, gpu_png=True, **kw)
        try:
            res[name] = pipe.process(blobs, opts)[0]
        finally:
            pipe.close()
    assert res["webp"][2:] == res["plain"][2:]
    assert res["plain"][2][:2] == b"\xff\xd8" or res["plain"][2][:8] == b"\x89PNG\r\n\x1a\n"
    assert res["plain"][3][:2] == b"\xff\xd8"
    for i in range(2):
        f = res["webp"][i]
        assert f[:4] == b"RIFF" and f[8:12] == b"WEBP"
        if res["plain"][i][:8] == b"\x89PNG\r\n\x1a\n":
            want = decode(res["plain"][i])
        else:  # the device pixels before JPEG coding: the same batch, pixels out
            src, pseudo = decode_ex(blobs[i])
            op = ImageProcessor(OptionsBag(opts[i]), src.shape[1], src.shape[0]).to_op()
            if pseudo:
                op.flags |= L.FI_SRC_PSEUDOCLASS
            want = ctx.process([np.ascontiguousarray(src)], [op])[0][0]
        want = want if want.ndim == 3 else want[..., None]
        assert want.shape[1] == 100
        check_file(f, np.ascontiguousarray(want), literal=False)
    assert res["plain"][1][:2] == b"\xff\xd8"  # the opaque output without the switch: the option is ignored


def test_webp_encode_300_tiny_images_cross_the_scan_chunk(ctx):
    """One call of 300 images of 3 x 2 pixels, 1..4 channels in turn: the
    images are the items of the batch's scan (enc_scan_items), so 300 of them
    cross its 256-item chunk.  Their file lengths differ, and a RIFF file has an
    even length, so the packed files start at both alignments a WebP file can
    have, 0 and 2 mod 4, on either side of the chunk (the byte head and tail
    of enc_copy_aligned; the odd alignments are the JPEG and PNG tests')."""
    rng = np.random.default_rng(300)
    images = [rng.integers(0, 256, (2, 3, 1 + k % 4), dtype=np.uint8) for k in range(300)]
    files = ctx.webp_encode_host(images)
    assert all(f is not None for f in files)
    starts = np.concatenate([[0], np.cumsum([len(f) for f in files])])[:-1]
    assert {int(s) % 4 for s in starts[:256]} == {0, 2} and {int(s) % 4 for s in starts[256:]} == {0, 2}
    assert len({len(f) for f in files}) > 4
    for k, (px, f) in enumerate(zip(images, files)):
        assert f == webp_encode_host_form(px, -1), k
