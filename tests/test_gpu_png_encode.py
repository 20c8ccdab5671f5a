"""GPU PNG encode (fi_png_enc.hip).  PNG is lossless, so the check is exact:
every file is parsed by hand (signature, IHDR, chunk order, every CRC against
zlib.crc32), its IDAT payload inflated by zlib to the very end, and Pillow
must return the input pixels bit for bit.  On top: the adaptive filter choice
against a numpy restatement of its rule, the deflate quality against zlib's
Huffman-only coding of the same filtered stream, strided views, mixed batches
with rejected images, the capacity rule, the pipeline switch and the kernel
statistics.  Crafted content -- deep codes, the length and distance ladders,
the three block forms -- is in tests/_lossless_content.py and
tests/test_gpu_lossless_content.py."""
import io
import os
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

from flyimg_amd import _lib as L
from flyimg_amd.runtime import Context, png_encode_bound
from flyimg_amd.synth import synth_rgb

from ._png_files import deflate_matches as _deflate_matches

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAND = 32768
MODES = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _channels(rgb, c):
    """A c-channel image of an RGB one: gray, gray + alpha, RGB, RGB + alpha (the alpha a ramp)."""
    h, w = rgb.shape[:2]
    alpha = ((np.arange(w)[None, :] * 3 + np.arange(h)[:, None] * 5) & 255).astype(np.uint8)
    if c == 1:
        return np.ascontiguousarray(rgb[..., 1])
    if c == 2:
        return np.dstack([rgb[..., 1], alpha])
    if c == 3:
        return rgb
    return np.dstack([rgb, alpha])


def _parse(blob, px):
    """Every check of one file; returns (IDAT payload, filtered stream)."""
    px3 = px if px.ndim == 3 else px[..., None]
    h, w, c = px3.shape
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(blob):
        n, typ = struct.unpack(">I4s", blob[pos:pos + 8])
        data = blob[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", blob[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(typ + data), (typ, len(chunks))
        chunks.append((typ, data))
        pos += 12 + n
    assert pos == len(blob)
    types = [t for t, _ in chunks]
    assert types[0] == b"IHDR" and types[-1] == b"IEND" and len(types) >= 3
    assert all(t == b"IDAT" for t in types[1:-1]) and chunks[-1][1] == b""
    assert chunks[0][1] == struct.pack(">IIBBBBB", w, h, 8, {1: 0, 2: 4, 3: 2, 4: 6}[c], 0, 0, 0)
    payload = b"".join(d for t, d in chunks if t == b"IDAT")
    assert payload[0] == 0x78 and (payload[0] * 256 + payload[1]) % 31 == 0 and not payload[1] & 0x20
    z = zlib.decompressobj()
    stream = z.decompress(payload)
    assert z.eof and z.unused_data == b""
    assert len(stream) == h * (w * c + 1)
    im = Image.open(io.BytesIO(blob))
    im.load()
    assert im.mode == MODES[c]
    assert np.array_equal(np.asarray(im).reshape(h, w, c), px3)
    assert len(blob) <= png_encode_bound(w, h, c)
    return payload, stream


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def _filter_types(px):
    """The rule of fi_png_encode_device's filter -1, restated: per row the
    type with the lowest sum of min(x, 256 - x), ties to the lower type."""
    px3 = (px if px.ndim == 3 else px[..., None]).astype(np.int64)
    h, w, c = px3.shape
    cur = px3.reshape(h, w * c)
    a = np.zeros_like(cur)
    a[:, c:] = cur[:, :-c]
    b = np.zeros_like(cur)
    b[1:] = cur[:-1]
    cc = np.zeros_like(cur)
    cc[1:, c:] = cur[:-1, :-c]
    cand = [cur, cur - a, cur - b, cur - (a + b) // 2, cur - _paeth(a, b, cc)]
    cost = np.stack([np.minimum(x & 255, 256 - (x & 255)).sum(axis=1) for x in cand])
    return np.argmin(cost, axis=0)  # (the first minimum: the lower type)


def _types(stream, px):
    px3 = px if px.ndim == 3 else px[..., None]
    h, w, c = px3.shape
    return np.frombuffer(stream, np.uint8).reshape(h, w * c + 1)[:, 0]


def _huffman_only(stream):
    z = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_HUFFMAN_ONLY)
    return len(z.compress(stream) + z.flush())


def _check(ctx, images, filter=-1, quality=True):
    files = ctx.png_encode_host(images, filter)
    out = []
    for k, (f, px) in enumerate(zip(files, images)):
        assert f is not None, k
        payload, stream = _parse(f, px)
        fl = filter[k] if isinstance(filter, (list, tuple)) else filter
        t = _types(stream, px)
        if fl < 0:
            assert np.array_equal(t, _filter_types(px)), k
        else:
            assert np.all(t == fl), k
        if quality:
            assert len(payload) <= _huffman_only(stream), (k, len(payload), _huffman_only(stream))
        out.append((f, payload, stream))
    return out


SIZES = [(1, 1), (1, 7), (7, 1), (3, 5), (63, 2), (64, 2), (65, 2)]


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_png_encode_small_geometries(ctx, w, h):
    """Row bytes on either side of a wave, every channel count, adaptive and
    every fixed filter."""
    rgb = synth_rgb(w, h, 3 + w + h)
    images = [_channels(rgb, c) for c in (1, 2, 3, 4)]
    _check(ctx, images, -1)
    _check(ctx, images * 5, [k for k in range(5) for _ in range(4)])


@pytest.mark.parametrize("w,h,chans", [(90, 91, (4,)), (200, 200, (4, 2)), (333, 211, (3, 1))],
                         ids=["90x91", "200x200", "333x211"])
def test_png_encode_bands(ctx, w, h, chans):
    """90x91 RGBA: 32,851 bytes, 83 past the first band; 200x200 RGBA: 5
    bands; 333x211 RGB: 7 bands."""
    rgb = synth_rgb(w, h, 40 + w)
    images = [_channels(rgb, c) for c in chans]
    res = _check(ctx, images, -1)
    nb = -(-len(res[0][2]) // BAND)
    assert nb == {90: 2, 200: 5, 333: 7}[w]
    assert res[0][0].count(b"IDAT") >= nb
    _check(ctx, images[:1], 4)


def test_png_encode_flat_and_checkerboard(ctx):
    """All-zero and one-colour images (length-258 matches, runs longer than a
    band), a two-colour checkerboard."""
    zero = np.zeros((200, 200, 4), np.uint8)
    one = np.empty((211, 333, 3), np.uint8)
    one[:] = (200, 30, 77)
    yy, xx = np.mgrid[0:120, 0:150]
    board = np.where(((xx + yy) & 1)[..., None] == 1, np.uint8(255), np.uint8(16)).astype(np.uint8).repeat(4, axis=2)
    board = np.ascontiguousarray(board)
    board[..., 3] = 255
    gray = np.full((300, 300), 99, np.uint8)
    res = _check(ctx, [zero, one, board, gray], -1)
    _check(ctx, [zero, one, board, gray], 0)
    assert len(res[0][0]) < 2000 and len(res[3][0]) < 2000  # runs: a few hundred symbols per band


def test_png_encode_golden_square(ctx):
    """tests/golden/square-opaque-200.png, as RGBA and as it is stored."""
    im = Image.open(os.path.join(GOLDEN, "square-opaque-200.png"))
    rgba = np.ascontiguousarray(np.asarray(im.convert("RGBA")))
    rgb = np.ascontiguousarray(rgba[..., :3])
    res = _check(ctx, [rgba, rgb], -1)
    assert len(set(_types(res[0][2], rgba).tolist())) >= 2


def test_png_encode_noise_is_stored_within_the_bound(ctx):
    rng = np.random.default_rng(2)
    images = [rng.integers(0, 256, (157, 211, 4), dtype=np.uint8), rng.integers(0, 256, (5, 3, 2), dtype=np.uint8),
              rng.integers(0, 256, (128, 256), dtype=np.uint8)]
    files = ctx.png_encode_host(images, 0)
    for f, px in zip(files, images):
        payload, stream = _parse(f, px)  # (checks len(f) <= png_encode_bound)
        assert len(f) > len(stream)      # nothing to gain: stored blocks


def test_png_encode_match_distances(ctx):
    """filter 0 on a raw pattern of period 3 (the shortest distances) and on one
    whose bands end with a repeat of their own first bytes, 32,742 bytes back
    (a distance at the edge of the band: distance symbol 29 with 13 extra
    bits, a 40-bit-and-more value in the bit buffer).  A period of 32,768 - 3
    itself leaves nothing to match: a band's window is the band, so only its
    last 3 bytes have a partner, and the type bytes at every multiple of 256
    break even that; hence the repeat is laid into the real stream, behind the
    type bytes.  The inflated symbols must hold that match in every band."""
    w, h = 255, 384  # rows of 256 bytes with the type byte: 128 rows are a band, 3 bands
    p3 = np.resize(np.array([17, 200, 91], np.uint8), 260 * w).reshape(260, w)
    rng = np.random.default_rng(4)
    far = rng.integers(1, 17, (h, w), dtype=np.uint8)  # 4 bits a byte: dynamic codes, no chance matches that pay
    shift, run = 230, 25
    dist = 127 * 256 + shift
    for b in range(3):
        far[128 * b, :run] = rng.integers(100, 256, run, dtype=np.uint8)  # values found nowhere else
        far[128 * b + 127, shift:] = far[128 * b, :run]
    assert dist == 32742 and shift + run == w
    res = _check(ctx, [p3, far], 0)
    # period 3 (and, with the type bytes, 256): long matches -- a row of 256 bytes takes at most
    # three symbols of at most 48 bits, 18 bytes
    assert len(res[0][1]) < len(res[0][2]) // 14
    blocks, total = _deflate_matches(res[0][1])
    assert total == len(res[0][2]) and min(d for m in blocks for _, d in m) <= 256
    blocks, total = _deflate_matches(res[1][1])
    assert total == len(res[1][2])
    # every band's block carries the repeat (the empty stored blocks between them hold nothing); the
    # hash table keeps one candidate per bucket, so the match may begin some bytes into the run
    far_runs = [max((ln for ln, d in m if d == dist), default=0) for m in blocks if m]
    print("far matches (length per band):", far_runs)
    assert len(far_runs) == 3 and all(3 <= x <= run for x in far_runs), far_runs


def test_png_encode_adaptive_filter_picks_several_types(ctx):
    """The photograph-like input picks more than one filter type over its rows
    (each row's type is checked against the restated rule in _check)."""
    px = _channels(synth_rgb(500, 375, 1), 4)
    (f, payload, stream), = _check(ctx, [px], -1)
    counts = np.bincount(_types(stream, px), minlength=5)
    assert counts.sum() == 375 and (counts > 0).sum() >= 2, counts


def test_png_encode_strided_view(ctx):
    """A sub-rectangle of a larger device image: pointer offset, stride larger
    than the width, a start that is not 16-byte aligned."""
    big = _channels(synth_rgb(300, 200, 21), 4)
    p = ctx.malloc(big.nbytes)
    try:
        ctx.h2d(p, big)
        x0, y0, w, h = 27, 13, 181, 95
        view = (p + y0 * 1200 + x0 * 4 + 0, w, h, 1200, 4)
        odd = (p + y0 * 1200 + x0 * 4 + 1, 33, 40, 1200, 1)  # a gray view starting on an odd byte
        assert view[0] % 16 != 0 and odd[0] % 2 == 1
        got = ctx.png_encode([view, odd, view], [-1, -1, 3])
    finally:
        ctx.free(p)
    sl = np.ascontiguousarray(big[y0:y0 + h, x0:x0 + w])
    flat = big.reshape(200, 1200)
    sl1 = np.ascontiguousarray(flat[y0:y0 + 40, x0 * 4 + 1:x0 * 4 + 1 + 33])
    _, s0 = _parse(got[0], sl)
    assert np.array_equal(_types(s0, sl), _filter_types(sl))
    _parse(got[1], sl1)
    _, s2 = _parse(got[2], sl)
    assert np.all(_types(s2, sl) == 3)


def test_png_encode_mixed_batch_with_rejected_images(ctx):
    """One call: sizes, channel counts and filters mixed; 5 channels, width 0
    and filter 7 get FI_EINVAL, the return code is the first failing status,
    the other files are intact."""
    rgb = [synth_rgb(w, h, 30 + i) for i, (w, h) in enumerate(
        [(120, 80), (31, 45), (64, 64), (200, 8), (8, 200), (77, 55), (130, 129), (24, 40)])]
    images = [_channels(r, 1 + i % 4) for i, r in enumerate(rgb)]
    filters = [-1, 0, 1, 2, 3, 4, -1, -1]
    ptrs = [ctx.malloc(a.nbytes) for a in images]
    try:
        views = []
        for a, p in zip(images, ptrs):
            ctx.h2d(p, a)
            c = a.shape[2] if a.ndim == 3 else 1
            views.append((p, a.shape[1], a.shape[0], a.shape[1] * c, c))
        bad = [(ptrs[0], 10, 10, 50, 5), (ptrs[0], 0, 10, 40, 4), (ptrs[0], 10, 10, 40, 4)]
        order = views[:3] + bad[:1] + views[3:6] + bad[1:] + views[6:]
        fl = filters[:3] + [-1] + filters[3:6] + [-1, 7] + filters[6:]
        rc, status, lens, bufs = ctx.png_encode_raw(order, fl)
    finally:
        for p in ptrs:
            ctx.free(p)
    assert rc == L.FI_EINVAL
    good = [0, 1, 2, 4, 5, 6, 9, 10]
    assert [status[i] for i in (3, 7, 8)] == [L.FI_EINVAL] * 3 and [lens[i] for i in (3, 7, 8)] == [0, 0, 0]
    for k, i in enumerate(good):
        assert status[i] == L.FI_OK, i
        _, stream = _parse(bufs[i][:lens[i]].tobytes(), images[k])
        t = _types(stream, images[k])
        assert np.array_equal(t, _filter_types(images[k])) if filters[k] < 0 else np.all(t == filters[k]), k
        assert np.all(bufs[i][lens[i]:][-64:] == 0xA5)


def test_png_encode_null_filter_is_adaptive(ctx):
    px = _channels(synth_rgb(70, 50, 6), 4)
    p = ctx.malloc(px.nbytes)
    try:
        ctx.h2d(p, px)
        rc, status, lens, bufs = ctx.png_encode_raw([(p, 70, 50, 280, 4)], None)
    finally:
        ctx.free(p)
    assert rc == L.FI_OK and status == [L.FI_OK]
    _, stream = _parse(bufs[0][:lens[0]].tobytes(), px)
    assert np.array_equal(_types(stream, px), _filter_types(px))


def test_png_encode_capacity(ctx):
    """out_cap one byte short: FI_ENOMEM with the true length, the guard bytes
    behind the capacity untouched, the neighbour encoded; a second call with
    the reported size succeeds."""
    a, b = _channels(synth_rgb(90, 70, 1), 4), _channels(synth_rgb(50, 60, 2), 2)
    ptrs = [ctx.malloc(x.nbytes) for x in (a, b)]
    try:
        ctx.h2d(ptrs[0], a)
        ctx.h2d(ptrs[1], b)
        views = [(ptrs[0], 90, 70, 360, 4), (ptrs[1], 50, 60, 100, 2)]
        rc, status, lens, bufs = ctx.png_encode_raw(views)
        assert rc == L.FI_OK
        ref_a, ref_b = bufs[0][:lens[0]].tobytes(), bufs[1][:lens[1]].tobytes()
        cap = len(ref_a) - 1
        rc, status, lens, bufs = ctx.png_encode_raw(views, caps=[cap, len(ref_b)])
        assert rc == L.FI_ENOMEM and status == [L.FI_ENOMEM, L.FI_OK]
        assert lens == [len(ref_a), len(ref_b)]
        assert bufs[0].size == cap + 64 and np.all(bufs[0][cap:] == 0xA5)  # the guard bytes behind out_cap
        assert bufs[1][:lens[1]].tobytes() == ref_b and np.all(bufs[1][lens[1]:] == 0xA5)
        rc, status, lens, bufs = ctx.png_encode_raw(views[:1], caps=[lens[0]])
        assert rc == L.FI_OK and status == [L.FI_OK] and bufs[0][:lens[0]].tobytes() == ref_a
    finally:
        for p in ptrs:
            ctx.free(p)
    _parse(ref_a, a)
    _parse(ref_b, b)


def test_png_encode_kernel_stats(ctx):
    ctx.set_timing(1)
    ctx.reset_stats()
    try:
        ctx.png_encode_host([_channels(synth_rgb(64, 48, 1), 4)])
        for name in ("k_png_filter", "k_png_lz", "k_png_emit", "k_png_pack"):
            ms, launches, _ = ctx.stats(name)
            assert launches == 1 and ms > 0, name
    finally:
        ctx.set_timing(0)
        ctx.reset_stats()


def test_codec_pipeline_gpu_png(ctx):
    """RGBA PNG sources at w_120: gpu_png writes PNG files of the pixels the
    host writer's files hold; without gpu_png the gpu_encode pipeline writes
    byte for byte what the default pipeline writes."""
    from flyimg_amd.codec import CodecPipeline, decode

    blobs = []
    for k, (w, h) in enumerate([(200, 150), (333, 211), (121, 240)]):
        b = io.BytesIO()
        Image.fromarray(_channels(synth_rgb(w, h, 50 + k), 4)).save(b, "PNG")
        blobs.append(b.getvalue())
    b = io.BytesIO()
    Image.fromarray(synth_rgb(160, 120, 60)).save(b, "JPEG", quality=90)
    blobs.append(b.getvalue())  # a JPEG output in the same batch
    opts = ["w_120"] * 4
    res = {}
    for name, kw in (("png", dict(gpu_encode=True, gpu_png=True)), ("enc", dict(gpu_encode=True)), ("host", {})):
        pipe = CodecPipeline(ctx, threads=4, **kw)
        try:
            res[name] = pipe.process(blobs, opts)[0]
        finally:
            pipe.close()
    assert res["enc"][:3] == res["host"][:3]  # gpu_png off: the host writer's files
    assert res["png"][3] == res["enc"][3] and res["png"][3][:2] == b"\xff\xd8"
    for i in range(3):
        assert res["png"][i][:8] == b"\x89PNG\r\n\x1a\n" and res["png"][i] != res["enc"][i]
        want = decode(res["enc"][i])
        assert want.shape[2] == 4 and want.shape[1] == 120
        _parse(res["png"][i], want)


def test_png_encode_bands_across_the_scan_chunk(ctx):
    """One call of 254 images of 4 x 4, a gray 300 x 220 image and 300 more of
    4 x 4: the gray image's filtered stream is 66,220 bytes = 3 bands, the
    items 254..256 of the batch's scan (enc_scan_items) on either side of its
    first 256-item chunk; 557 bands cross the second.  Every file decodes to
    its pixels and is the file the image gives in a call of its own."""
    rgb = synth_rgb(4, 4 * 8, 77)
    small = [_channels(np.ascontiguousarray(rgb[4 * k:4 * k + 4]), 1 + k % 4) for k in range(8)]
    big = np.ascontiguousarray(synth_rgb(300, 220, 78)[..., 1])
    assert 220 * (300 + 1) == 66220 and -(-66220 // BAND) == 3
    images = [small[k % 8] for k in range(254)] + [big] + [small[(k + 3) % 8] for k in range(300)]
    alone = {a.tobytes(): ctx.png_encode_host([a])[0] for a in small + [big]}
    files = ctx.png_encode_host(images)
    assert len(files) == 555
    for k, (a, f) in enumerate(zip(images, files)):
        assert f is not None and f == alone[a.tobytes()], k
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))), a), k
