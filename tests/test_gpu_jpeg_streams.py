"""GPU JPEG decode of the hand-built and damaged streams of tests/_jpeg_files.py
against libjpeg-turbo through Pillow.

Corpus A (well-formed streams Pillow's encoder never writes): every image
decodes on the GPU, bit-exact, one call per group -- no fallback.
Corpus B (damaged streams libjpeg still decodes): every image is bit-exact or
comes back FI_EUNSUPPORTED (None) with the rest of its batch unaffected --
never FI_EINVAL, never another picture; the streams whose picture does not
depend on the damage must decode.  The test prints how many fell back (when
written: 47 of 248 baseline streams -- 17 in the parse for their restart
markers, 30 for coefficients outside the IDCTs' common range -- and 20 of 31
progressive ones -- 12 in the parse, 8 for a symbol outside its scan's band)."""
import io

import numpy as np
import pytest
from PIL import Image

from flyimg_amd import _lib as L
from flyimg_amd.runtime import Context

from tests import _jpeg_files as J

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _ref(blob):
    return np.asarray(Image.open(io.BytesIO(blob)))


@pytest.mark.parametrize("group", list(J.corpus_a()))
def test_corpus_a_bit_exact_without_fallback(ctx, group):
    cases = J.corpus_a()[group]
    outs = ctx.jpeg_decode_host([c.file.stream for c in cases])
    for c, got in zip(cases, outs):
        assert got is not None, f"{c.name}: handed to the host"
        ref = _ref(c.file.stream)
        assert got.shape == ref.shape, c.name
        assert np.array_equal(got, ref), f"{c.name}: {(got != ref).sum()} of {ref.size} values differ"


def _status(ctx, blobs, progressive):
    ptrs = [ctx.malloc(72 * 100 * 3) for _ in blobs]
    try:
        return ctx.jpeg_decode(blobs, ptrs, [100 * 3] * len(blobs), progressive=progressive)
    finally:
        for p in ptrs:
            ctx.free(p)


@pytest.mark.parametrize("progressive", [False, True], ids=["baseline", "progressive"])
def test_corpus_b_bit_exact_or_handed_to_the_host(ctx, progressive):
    cases = [d for d in J.corpus_b() if d.progressive == progressive]
    blobs = [d.blob for d in cases]
    outs = ctx.jpeg_decode_host(blobs, progressive=progressive)
    fell = [d.name for d, got in zip(cases, outs) if got is None]
    print(f"corpus B ({'progressive' if progressive else 'baseline'}): {len(fell)} of {len(cases)} handed to the host: "
          f"{fell}")
    for d, got in zip(cases, outs):
        if got is None:
            assert not d.must_decode, f"{d.name}: libjpeg's picture does not depend on the damage"
            continue
        ref = _ref(d.blob)
        assert got.shape == ref.shape, d.name
        assert np.array_equal(got, ref), f"{d.name}: {(got != ref).sum()} of {ref.size} values differ"
    # a stream handed over is FI_EUNSUPPORTED, never FI_EINVAL (all of these are at most 97 x 72)
    st = _status(ctx, blobs, progressive)
    assert set(st) <= {L.FI_OK, L.FI_EUNSUPPORTED}, [(d.name, s) for d, s in zip(cases, st) if s not in (0, -5)]
    assert [s != 0 for s in st] == [got is None for got in outs]


def test_corpus_b_through_codec_pipeline(ctx):
    """A dozen damaged blobs and two intact ones: the pipeline with the GPU
    decoder returns the encoded outputs and records of the host-decode pipeline."""
    from flyimg_amd.codec import CodecPipeline

    by = {d.name: d.blob for d in J.corpus_b()}
    names = ["cut_444_50", "cut_420_25", "cut_w420_90", "cut_on_mcu_boundary", "grey_dri4_interval_cut",
             "w420_dri2_interval_cut", "grey_dri4_marker_plus_2", "w420_dri2_marker_lost",
             "grey_dri4_marker_after_last_mcu", "w420_dri2_surplus_before_marker", "sixteen_ones_dc_1",
             "sixteen_ones_ac_no_dri"]
    names += [n for n in by if n.startswith("flip_420")][:2]
    blobs = [by[n] for n in names] + [J.flip_sources()["420_33x17"], J.corpus_a()["framing"][0].file.stream]
    opts = ["w_20", "w_16,h_16,c_1", "w_24,q_80"]
    opts = [opts[i % 3] for i in range(len(blobs))]
    res = {}
    for gd in (True, False):
        pipe = CodecPipeline(ctx, threads=4, gpu_decode=gd)
        try:
            res[gd] = pipe.process(blobs, opts)
        finally:
            pipe.close()
    (ea, ra), (eb, rb) = res[True], res[False]
    assert ea == eb
    key = ("out_w", "out_h", "crop_x", "crop_y", "crop_w", "crop_h", "status")
    assert [[getattr(r, k) for k in key] for r in ra] == [[getattr(r, k) for k in key] for r in rb]
