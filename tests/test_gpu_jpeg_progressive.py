"""GPU decode of progressive JPEG sources (k_jpeg_prog, opt-in through
fi_jpeg_decode_device_ex + FI_JPEG_PROGRESSIVE) against libjpeg-turbo through
Pillow: every comparison is np.array_equal with Pillow's decode of the same
bytes.  Pillow's own scan script (10 scans, 3 levels, successive
approximation), restart intervals inside progressive scans, the scan scripts
of other encoders (the golden files), a batch mixing baseline, progressive and
unsupported streams, the flag's semantics and the codec pipeline's switch."""
import io
import os

import numpy as np
import pytest
from PIL import Image, ImageFile

from flyimg_amd import _lib as L
from flyimg_amd.runtime import Context, jpeg_info, jpeg_scan_info
from flyimg_amd.synth import synth_rgb

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _enc(img, **kw):
    """Pillow's encoder buffer is too small for a dense progressive file: widen it for the call."""
    b = io.BytesIO()
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, 4 * img.size + 65536)
    try:
        Image.fromarray(img).save(b, "JPEG", **kw)
    finally:
        ImageFile.MAXBLOCK = old
    return b.getvalue()


def _ref(blob):
    return np.asarray(Image.open(io.BytesIO(blob)))


def _golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _check(ctx, blob, name=""):
    ref = _ref(blob)
    got = ctx.jpeg_decode_host([blob], progressive=True)[0]
    assert got is not None and got.shape == ref.shape, name
    assert np.array_equal(got, ref), f"{name}: {(got != ref).sum()} of {ref.size} values differ"


CASES = []
for ss in (0, 1, 2):
    for (w, h) in ((1, 1), (7, 9), (17, 33), (65, 33), (333, 211)):
        CASES.append((f"ss{ss}_{w}x{h}", w, h, dict(quality=90, subsampling=ss)))
CASES += [
    ("ss2_q30", 300, 200, dict(quality=30, subsampling=2)),
    ("ss2_q100", 300, 200, dict(quality=100, subsampling=2)),
    ("ss1_restart_1", 65, 33, dict(quality=90, subsampling=1, restart_marker_blocks=1)),
    ("ss2_restart_blocks", 250, 130, dict(quality=90, subsampling=2, restart_marker_blocks=5)),
    ("ss0_restart_rows", 97, 61, dict(quality=90, subsampling=0, restart_marker_rows=1)),
    ("ss2_1920x1080", 1920, 1080, dict(quality=90, subsampling=2)),
]


@pytest.mark.parametrize("name,w,h,kw", CASES, ids=[c[0] for c in CASES])
def test_progressive_decode_bit_exact(ctx, name, w, h, kw):
    blob = _enc(synth_rgb(w, h, 11 + w + h), progressive=True, **kw)
    assert jpeg_info(blob) is None and jpeg_info(blob, progressive=True) == (w, h, 3)
    assert jpeg_scan_info(blob)[3:] == (10, 3)
    _check(ctx, blob, name)


@pytest.mark.parametrize("w,h", [(1, 1), (33, 17), (97, 61)])
def test_progressive_decode_gray_bit_exact(ctx, w, h):
    blob = _enc(synth_rgb(w, h, 3)[..., 1].copy(), quality=90, progressive=True)
    assert jpeg_scan_info(blob) == (w, h, 1, 6, 3)
    _check(ctx, blob)


@pytest.mark.parametrize("ss", [0, 2])
def test_progressive_decode_noise_bit_exact(ctx, ss):
    """Uniform noise at q97: large coefficients, dense refinement bits, 0xFF stuffing."""
    px = np.random.default_rng(ss).integers(0, 256, (157, 211, 3), dtype=np.uint8)
    _check(ctx, _enc(px, quality=97, subsampling=ss, progressive=True))


def test_progressive_decode_flat_long_eobrun(ctx):
    """Flat 333x211 at q30: end-of-band runs over more than 1000 blocks."""
    _check(ctx, _enc(np.full((211, 333, 3), (200, 90, 30), np.uint8), quality=30, progressive=True))
    _check(ctx, _enc(np.full((211, 333), 77, np.uint8), quality=30, progressive=True))


@pytest.mark.parametrize("name", ["smart_crop.jpg", "faces.jpg", "extract-result.jpg"])
def test_progressive_decode_golden_files(ctx, name):
    """Other encoders' scan scripts: non-interleaved DC scans without
    successive approximation (smart_crop), four-step AC refinement (faces)."""
    _check(ctx, _golden(name), name)


def test_progressive_mixed_batch(ctx):
    """One call: baseline, progressive, CMYK (unsupported), truncated
    progressive (unsupported), progressive gray to 3 channels, and six more
    progressive images of different content (optimised tables: far more than
    8 distinct Huffman tables in the batch)."""
    px = synth_rgb(123, 77, 5)
    cmyk = io.BytesIO()
    Image.fromarray(px).convert("CMYK").save(cmyk, "JPEG", progressive=True)
    prog = _enc(px, quality=85, subsampling=2, progressive=True)
    blobs = [_enc(px, quality=90, subsampling=2), prog, cmyk.getvalue(), prog[:len(prog) // 2],
             _enc(px[..., 0].copy(), quality=80, progressive=True)]
    for k in range(6):
        blobs.append(_enc(synth_rgb(61 + 16 * k, 47 + 9 * k, 100 + k), quality=60 + 7 * k, subsampling=k % 3,
                          progressive=True))
    infos = [jpeg_info(b, progressive=True) for b in blobs]
    assert infos[2] is None and infos[3] is None
    dims = [i if i else (1, 1, 3) for i in infos]
    ptrs = [ctx.malloc(w * h * 3) for w, h, _ in dims]
    try:
        status = ctx.jpeg_decode(blobs, ptrs, [w * 3 for w, _, _ in dims], channels=3, progressive=True)
        want = [0, 0, L.FI_EUNSUPPORTED, L.FI_EUNSUPPORTED] + [0] * 7
        assert status == want
        for i, (b, (w, h, _), p) in enumerate(zip(blobs, dims, ptrs)):
            if want[i]:
                continue
            got = ctx.d2h(p, w * h * 3).reshape(h, w, 3)
            assert np.array_equal(got, np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))), i
    finally:
        for p in ptrs:
            ctx.free(p)


def test_progressive_flag_semantics_and_kernel_stats(ctx):
    blob = _enc(synth_rgb(65, 33, 9), quality=90, subsampling=2, progressive=True)
    p = ctx.malloc(65 * 33 * 3)
    try:
        assert ctx.jpeg_decode([blob], [p], [65 * 3]) == [L.FI_EUNSUPPORTED]  # flags = 0: as before
        ctx.set_timing(True)
        try:
            assert ctx.jpeg_decode([blob], [p], [65 * 3], progressive=True) == [0]
            ms, n, _ = ctx.stats("k_jpeg_prog")
            assert n > 0 and ms > 0
        finally:
            ctx.set_timing(False)
        assert np.array_equal(ctx.d2h(p, 65 * 33 * 3).reshape(33, 65, 3), _ref(blob))
    finally:
        ctx.free(p)


def test_pipeline_gpu_progressive_matches_host_path(ctx):
    from flyimg_amd.codec import CodecPipeline, gpu_decodable

    blobs = [_golden("smart_crop.jpg"), _enc(synth_rgb(640, 481, 21), quality=90, subsampling=2, progressive=True)]
    assert all(gpu_decodable(b) is None for b in blobs)
    assert [gpu_decodable(b, progressive=True) for b in blobs] == [(1000, 750, 3), (640, 481, 3)]
    opts = ["w_500,smc_1", "w_300,h_250,c_1"]
    off = CodecPipeline(ctx, threads=2)
    on = CodecPipeline(ctx, threads=2, gpu_progressive=True)
    try:
        out0, rec0 = off.process(blobs, opts)
        out1, rec1 = on.process(blobs, opts)
    finally:
        off.close()
        on.close()
    assert [bytes(a) for a in out0] == [bytes(b) for b in out1]
    key = ("out_w", "out_h", "out_channels", "crop_x", "crop_y", "crop_w", "crop_h", "crop_score", "status")
    assert [[getattr(r, k) for k in key] for r in rec0] == [[getattr(r, k) for k in key] for r in rec1]
