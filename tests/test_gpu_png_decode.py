"""GPU PNG decode (fi_png_dec.hip): pixels must equal Pillow's reading of the
file bit for bit (``convert("RGB")`` / ``convert("RGBA")``, or the natural mode
for ``out_channels`` 0); for hand-built files, the numpy pixels the file was
built from.  Geometry around the wavefront's lane skew and band seams, every
filter and filter succession, zlib's levels and strategies and the
hand-assembled deflate blocks, the output channel rules, strides, a mixed batch
with malformed files (only ones the CPU driver has taken to an error status
under the sanitizers), and the codec pipeline's switch."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

from flyimg_amd import _lib as L
from flyimg_amd.codec import CodecPipeline, decode
from flyimg_amd.runtime import Context
from flyimg_amd.synth import synth_rgb

from . import _png_files as P
from .test_png_decode_cpu import LEVELS, STRATEGIES, hand_streams, malformed_files, zlib_stream

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 63, 64, 65, 200)   # lane-skew edges
HEIGHTS = (1, 2, 63, 64, 65, 129)  # band seams and the carry row
KINDS = ("gray", "rgb", "la", "rgba", "pal", "paltrns")
CT = {"gray": 0, "rgb": 2, "la": 4, "rgba": 6, "pal": 3, "paltrns": 3}


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _pillow(blob, oc=0):
    im = Image.open(io.BytesIO(blob))
    alpha = im.mode in ("RGBA", "LA", "PA") or (im.mode == "P" and "transparency" in im.info)
    if oc == 0 and im.mode != "P":
        return np.asarray(im)
    return np.asarray(im.convert("RGBA" if oc == 4 or (oc == 0 and alpha) else "RGB"))


def _pixels(kind, w, h, seed):
    """Pixels (or palette indices) of a picture with noise: every filter has work to do."""
    rng = np.random.default_rng(seed)
    rgb = synth_rgb(w, h, seed)
    a = rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
    if kind == "gray":
        return rgb[:, :, 1].copy()
    if kind == "rgb":
        return rgb
    if kind == "la":
        return np.dstack([rgb[:, :, 1:2], a])
    if kind == "rgba":
        return np.dstack([rgb, a])
    return rng.integers(0, 256, (h, w), dtype=np.uint8)  # indices, some beyond PLTE and tRNS


def _file(kind, px, types, level=6, **kw):
    rng = np.random.default_rng(px.shape[0] * 1000 + px.shape[1])
    if kind.startswith("pal"):
        kw["plte"] = rng.integers(0, 256, 3 * 200, dtype=np.uint8).tobytes()  # 200 entries: indices 200..255 lie beyond
        if kind == "paltrns":
            kw["trns"] = rng.integers(0, 256, 90, dtype=np.uint8).tobytes()
    h, w = px.shape[:2]
    return P.png_file(w, h, CT[kind], zlib.compress(P.filter_stream(px, types), level), **kw)


def _check(ctx, blobs, wants, ocs=None, names=None):
    got = ctx.png_decode_host(blobs, ocs)
    for k, (g, want) in enumerate(zip(got, wants)):
        assert g is not None, names[k] if names else k
        assert g.shape == want.shape and np.array_equal(g, want), names[k] if names else k


def test_geometry_cross(ctx):
    """Every width with every height; the six source kinds rotate so that each
    width and each height meets each kind.  Filter types are random per row."""
    blobs, wants, names = [], [], []
    for iw, w in enumerate(WIDTHS):
        for ih, h in enumerate(HEIGHTS):
            kind = KINDS[(iw + ih) % 6]
            rng = np.random.default_rng(100 * iw + ih)
            px = _pixels(kind, w, h, 7 + 10 * iw + ih)
            f = _file(kind, px, [int(t) for t in rng.integers(0, 5, h)])
            blobs.append(f)
            names.append((kind, w, h))
            want = _pillow(f)
            if not kind.startswith("pal"):
                assert np.array_equal(want, px), names[-1]  # the file is what it was built from
            wants.append(want)
    _check(ctx, blobs, wants, names=names)


def test_filters_each_type_and_every_succession_across_a_band_seam(ctx):
    blobs, wants, names = [], [], []
    kinds = ("gray", "la", "rgb", "rgba")
    for t in range(5):  # each type on every row
        for k, kind in enumerate(kinds):
            px = _pixels(kind, 37 + k, 70, 50 + t)
            blobs.append(_file(kind, px, [t] * 70))
            wants.append(px)
            names.append(("all", t, kind))
    for t1 in range(5):  # t1 on the band's last row (63), t2 on the next band's first (64)
        for t2 in range(5):
            kind = kinds[(t1 + t2) % 4]
            px = _pixels(kind, 9, 66, 300 + 5 * t1 + t2)
            types = [(y * 7 + t1) % 5 for y in range(66)]
            types[63], types[64] = t1, t2
            blobs.append(_file(kind, px, types))
            wants.append(px)
            names.append(("seam", t1, t2, kind))
    # one tall image in which every type follows every other, several seams
    seq = [a for t1 in range(5) for t2 in range(5) for a in (t1, t2)] * 3
    px = _pixels("rgba", 21, len(seq), 77)
    blobs.append(_file("rgba", px, seq))
    wants.append(px)
    names.append(("sequence",))
    _check(ctx, blobs, wants, names=names)


def test_paeth_ties_take_a_then_b_then_c(ctx):
    """Pixels from three values: a, b and c tie on most bytes, where the
    predictor's order decides."""
    blobs, wants = [], []
    for k, (kind, vals) in enumerate((("gray", (0, 1, 255)), ("rgba", (0, 128, 255)), ("rgb", (7, 7, 8)), ("la", (254, 255, 0)))):
        rng = np.random.default_rng(k)
        c = {"gray": 1, "la": 2, "rgb": 3, "rgba": 4}[kind]
        px = np.asarray(vals, np.uint8)[rng.integers(0, 3, (70, 33, c))]
        px = px[:, :, 0] if c == 1 else px
        f = _file(kind, px, [4] * 70)
        assert np.array_equal(_pillow(f), px)
        blobs.append(f)
        wants.append(px)
    _check(ctx, blobs, wants)


def test_deflate_levels_strategies_hand_blocks_and_split_idat(ctx):
    px = synth_rgb(97, 61, 3)
    stream = P.filter_stream(px, [y % 5 for y in range(61)])
    blobs, wants, names = [], [], []
    for level in LEVELS:
        for sname, strat in STRATEGIES.items():
            blobs.append(P.png_file(97, 61, 2, zlib_stream(stream, level, strat)))
            wants.append(px)
            names.append((level, sname))
    # a stream above 65,535 bytes at level 0: several stored blocks
    big = synth_rgb(160, 140, 5)
    blobs.append(P.png_file(160, 140, 2, zlib_stream(P.filter_stream(big, [1] * 140), 0, zlib.Z_DEFAULT_STRATEGY)))
    wants.append(big)
    names.append("stored blocks")
    for name, (z, data) in hand_streams().items():  # 255-pixel gray rows; Pillow reads them
        f = P.png_file(255, len(data) // 256, 0, z)
        blobs.append(f)
        wants.append(_pillow(f))
        names.append(name)
    z = zlib_stream(stream, 6, zlib.Z_DEFAULT_STRATEGY)
    blobs.append(P.png_file(97, 61, 2, z, split=[0, 1, 1, 0, 500, 1]))  # the zlib header across chunks, empty chunks
    wants.append(px)
    names.append("multi-IDAT")
    _check(ctx, blobs, wants, names=names)


def test_out_channels_per_source_kind(ctx):
    files = {k: _file(k, _pixels(k, 45, 67, 9), [y % 5 for y in range(67)]) for k in KINDS}
    alpha = {"la", "rgba", "paltrns"}
    blobs, ocs, wants = [], [], []
    for kind, f in files.items():
        for oc in (0, 3, 4):
            blobs.append(f)
            ocs.append(oc)
            wants.append(None if oc == 3 and kind in alpha else _pillow(f, oc))
    got = ctx.png_decode_host(blobs, ocs)
    for f, oc, g, want in zip(blobs, ocs, got, wants):
        if want is None:
            assert g is None
        else:
            assert g is not None and g.shape == want.shape and np.array_equal(g, want), oc
    # the statuses: FI_EINVAL for RGB from a source with alpha and for a channel count that is none
    p = ctx.malloc(45 * 67 * 4)
    try:
        for kind in alpha:
            assert ctx.png_decode([files[kind]], [p], [45 * 3], 3) == [L.FI_EINVAL]
        assert ctx.png_decode([files["rgb"]], [p], [45 * 4], 2) == [L.FI_EINVAL]
        assert ctx.png_decode([files["rgb"]], [p], [45 * 3 - 1], 3) == [L.FI_EINVAL]  # stride below the row
        assert ctx.png_decode([files["rgb"]], [p], [45 * 3], None) == [L.FI_OK]       # NULL array: natural
    finally:
        ctx.free(p)


def test_wide_stride_and_unaligned_destination(ctx):
    # (kind, w, h, out_channels, channels written, dst_stride, offset of dst from a 256-byte boundary)
    cases = [("rgba", 33, 70, 4, 4, 33 * 4 + 13, 1), ("rgb", 65, 66, 3, 3, 65 * 3 + 1, 3), ("gray", 64, 65, 0, 1, 100, 5),
             ("gray", 20, 10, 4, 4, 96, 2), ("pal", 31, 64, 0, 3, 31 * 3 + 7, 7)]
    blobs, ptrs, strides, ocs, wants = [], [], [], [], []
    size = 1 << 16
    base = ctx.malloc(size * len(cases))
    try:
        ctx.h2d(base, np.full(size * len(cases), 0xA5, np.uint8))
        for k, (kind, w, h, oc, nc, stride, off) in enumerate(cases):
            f = _file(kind, _pixels(kind, w, h, 40 + k), [y % 5 for y in range(h)])
            blobs.append(f)
            wants.append(_pillow(f, oc).reshape(h, w * nc))
            ptrs.append(base + k * size + 256 + off)
            strides.append(stride)
            ocs.append(oc)
        assert ctx.png_decode(blobs, ptrs, strides, ocs) == [L.FI_OK] * len(cases)
        mem = ctx.d2h(base, size * len(cases))
        for k, (kind, w, h, _, oc, stride, off) in enumerate(cases):
            slot = mem[k * size:(k + 1) * size]
            at = 256 + off
            assert (slot[:at] == 0xA5).all(), kind
            rows = slot[at:at + h * stride].reshape(h, stride)
            assert np.array_equal(rows[:, :w * oc], wants[k]), kind
            assert (rows[:-1, w * oc:] == 0xA5).all(), kind  # the padding is untouched
            assert (slot[at + (h - 1) * stride + w * oc:] == 0xA5).all(), kind
    finally:
        ctx.free(base)


def test_mixed_batch_statuses_and_neighbours(ctx):
    mf = malformed_files()
    goods = [_file(k, _pixels(k, 50, 66, 3 + i), [y % 5 for y in range(66)]) for i, k in enumerate(("rgba", "gray", "rgb"))]
    order = ["interlaced", "wrong Adler-32", "filter byte 5", "cut inside a dynamic block", "inflates to too many bytes"]
    blobs = [goods[0]]
    want_status = [L.FI_OK]
    for k, name in enumerate(order):
        blobs.append(mf[name][0])
        want_status.append(mf[name][1])
        blobs.append(goods[k % 3])
        want_status.append(L.FI_OK)
    assert [s for _, s in (mf[n] for n in order)] == [L.FI_EUNSUPPORTED] + [L.FI_EINVAL] * 4
    size = 40 * 71 * 4 + 50 * 66 * 4
    ptrs = [ctx.malloc(size) for _ in blobs]
    try:
        n = len(blobs)
        bufs = [L.ctypes.c_char_p(b) for b in blobs]
        data = (L.ctypes.c_void_p * n)(*[L.ctypes.cast(b, L.ctypes.c_void_p).value for b in bufs])
        lens = (L.ctypes.c_size_t * n)(*[len(b) for b in blobs])
        status = (L.ctypes.c_int32 * n)()
        rc = L.lib().fi_png_decode_device(ctx.h, data, lens, n, (L.ctypes.c_void_p * n)(*ptrs),
                                          (L.ctypes.c_int64 * n)(*[50 * 4] * n), None, status)
        assert list(status) == want_status
        assert rc == L.FI_EUNSUPPORTED  # the first failing status
        for k in range(0, n, 2):
            want = _pillow(blobs[k])
            got = ctx.d2h(ptrs[k], 66 * 200).reshape(66, 200)[:, :want[0].size]
            assert np.array_equal(got, want.reshape(66, -1)), k
    finally:
        for p in ptrs:
            ctx.free(p)


def _png(px, mode=None, **kw):
    b = io.BytesIO()
    im = Image.fromarray(px)
    (im.convert(mode) if mode else im).save(b, "PNG", **kw)
    return b.getvalue()


def _pipeline_sources():
    rgb = synth_rgb(240, 180, 12)
    a = ((np.arange(240)[None, :] * 3 + np.arange(180)[:, None] * 5) & 255).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(synth_rgb(200, 150, 2)).save(b, "JPEG", quality=88)
    pal = Image.fromarray(rgb).quantize(colors=64)
    pb = io.BytesIO()
    pal.save(pb, "PNG", transparency=3)
    return [_png(np.dstack([rgb, a])), _png(rgb), _png(rgb[:, :, 1]), _png(rgb, "P"), pb.getvalue(),
            _png(np.dstack([rgb[:, :, 0], a])), b.getvalue()]


OPTIONS = ["w_100", "w_120,h_70,c_1", "w_80", "w_90,h_90", "w_60", "w_100,r_90", "w_100"]


def test_pipeline_outputs_match_the_host_decode_arm(ctx):
    blobs = _pipeline_sources()
    ref = CodecPipeline(ctx, gpu_png_decode=False)
    dev = CodecPipeline(ctx, gpu_png_decode=True)
    try:
        want, _ = ref.process(blobs, OPTIONS)
        got, recs = dev.process(blobs, OPTIONS)
        assert ref.decode_stats == {"gpu": 1, "host": 6}
        assert dev.decode_stats == {"gpu": 7, "host": 0}  # every PNG on the GPU side
        for k, (g, w) in enumerate(zip(got, want)):
            assert g == w, k  # byte for byte
        assert [r.out_channels for r in recs][:3] == [4, 3, 3]
    finally:
        ref.close()
        dev.close()


def test_pipeline_device_resident_with_gpu_png(ctx):
    blobs = _pipeline_sources()
    ref = CodecPipeline(ctx, gpu_encode=True, gpu_png=True)
    dev = CodecPipeline(ctx, gpu_encode=True, gpu_png=True, gpu_png_decode=True)
    half = CodecPipeline(ctx, gpu_encode=True, gpu_png_decode=True)  # alpha outputs: down to the host PNG writer
    try:
        want, _ = ref.process(blobs, OPTIONS)
        got, _ = dev.process(blobs, OPTIONS)
        mid, _ = half.process(blobs, OPTIONS)
        assert dev.decode_stats == {"gpu": 7, "host": 0}
        for k, (g, m, w) in enumerate(zip(got, mid, want)):
            assert g[:4] == w[:4] == m[:4]  # the same container
            assert np.array_equal(decode(g), decode(w)), k
            assert np.array_equal(decode(m), decode(w)), k
        assert got[0][:4] == b"\x89PNG" and got[5][:4] == b"\x89PNG" and got[1][:2] == b"\xff\xd8"
    finally:
        ref.close()
        dev.close()
        half.close()


def test_pipeline_keeps_orientation_and_extracts_on_the_host(ctx):
    rgb = synth_rgb(120, 90, 5)
    ex = Image.Exif()
    ex[0x0112] = 6
    oriented = _png(rgb, exif=ex)
    assert b"eXIf" in oriented
    plain = _png(rgb)
    blobs = [oriented, plain, plain]
    opts = ["w_50", "e_1,p1x_10,p1y_5,p2x_100,p2y_80,w_40", "w_50"]
    ref = CodecPipeline(ctx)
    dev = CodecPipeline(ctx, gpu_png_decode=True)
    try:
        want, wr = ref.process(blobs, opts)
        got, gr = dev.process(blobs, opts)
        assert dev.decode_stats == {"gpu": 1, "host": 2}
        assert got == want
        assert (gr[0].out_w, gr[0].out_h) == (wr[0].out_w, wr[0].out_h) and gr[0].out_h > gr[0].out_w  # rotated
    finally:
        ref.close()
        dev.close()


def test_kernel_statistics(ctx):
    ctx.set_timing(True)
    try:
        ctx.reset_stats()
        f = _file("rgba", _pixels("rgba", 64, 64, 1), [4] * 64)
        assert ctx.png_decode_host([f, f])[0] is not None
        for name in ("k_png_inflate", "k_png_adler", "k_png_unfilter"):
            ms, n, _ = ctx.stats(name)
            assert n == 1 and ms > 0, name
    finally:
        ctx.set_timing(False)
