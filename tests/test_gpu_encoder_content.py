"""Both GPU JPEG encoders (fi_jpeg_enc.hip, fi_jpeg_penc.hip) on the crafted
content of tests/_encoder_content.py, byte for byte against libjpeg-turbo
through Pillow: Huffman trees libjpeg had to limit to 16 bits (k_jpeg_ptab),
every ZRL rule of the refinement scan and ZRL chains (k_jpeg_pstat,
k_jpeg_pcode, k_jpeg_henc), DC differences of +-2040, AC magnitudes of 512
and more on 16-bit codes, dense blocks, EOB runs of 4094 and 8188, and the
full-swing pixel corpus of tests/_adversarial.py through k_jpeg_fdct at
qualities 1, 50 and 100.  tests/test_encoder_content_cpu.py proves each
property on Pillow's files alone.  The library's decoders read the files as
Pillow does."""
import io

import numpy as np
import pytest
from PIL import Image

from flyimg_amd.runtime import Context, jpeg_encode_bound
from flyimg_amd.synth import synth_rgb

from . import _encoder_content as E
from .test_encoder_content_cpu import pillow_baseline
from .test_jpeg_penc_cpu import pillow_progressive, same as _same

pytestmark = pytest.mark.gpu

CRAFTED = E.crafted()
GROUPS = {
    "deep": ["deep17_gray", "deep17_444", "deep17_420", "deep18_gray"],
    "runs_swing": [n for n in CRAFTED if n.split("_")[0] in ("zero", "dc", "ac", "binary")],
    "long_eob": ["long_eob_flat", "long_eob_single"],
}


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _reference(c, progressive):
    return (pillow_progressive if progressive else pillow_baseline)(c.px, c.quality, c.subsampling)


def _encode_and_compare(ctx, cases, progressive):
    """one batched call; every file is Pillow's and within the bound"""
    got = ctx.jpeg_encode_host([c.px for c in cases], [c.quality for c in cases], [c.subsampling for c in cases],
                               progressive=progressive)
    bad = []
    for c, g in zip(cases, got):
        h, w = c.px.shape[:2]
        try:
            _same(g, _reference(c, progressive), c.name)
            assert len(g) <= jpeg_encode_bound(w, h, E.channels(c), c.quality, c.subsampling, progressive=progressive)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, f"{len(bad)} of {len(cases)}: " + "; ".join(bad[:8])
    return got


def test_groups_cover_every_crafted_case():
    assert sorted(sum(GROUPS.values(), [])) == sorted(CRAFTED)


@pytest.mark.parametrize("progressive", [False, True], ids=["baseline", "progressive"])
@pytest.mark.parametrize("group", list(GROUPS))
def test_crafted_content_byte_identical(ctx, group, progressive):
    _encode_and_compare(ctx, [CRAFTED[n] for n in GROUPS[group]], progressive)


@pytest.mark.parametrize("progressive", [False, True], ids=["baseline", "progressive"])
@pytest.mark.parametrize("q", E.PIXEL_QUALITIES)
def test_pixel_corpus_byte_identical(ctx, q, progressive):
    _encode_and_compare(ctx, list(E.pixel_corpus(q)), progressive)


def test_histograms_of_a_batch_are_independent(ctx):
    """deep17 first and last in one progressive batch, zero_runs and a smooth
    picture between them: every image gets the tables of its own symbols."""
    deep, runs = CRAFTED["deep17_gray"], CRAFTED["zero_runs_444"]
    smooth = E.Case("synth_rgb", synth_rgb(97, 61, 5), 75, 2, None)
    _encode_and_compare(ctx, [deep, runs, smooth, deep], True)


def _decode_and_compare(ctx, files, names, progressive):
    back = ctx.jpeg_decode_host(files, progressive=progressive)
    for n, f, got in zip(names, files, back):
        ref = np.asarray(Image.open(io.BytesIO(f)))
        assert got is not None, f"{n}: handed to the host"
        assert got.shape == ref.shape and np.array_equal(got, ref), n


def test_progressive_decoder_reads_the_crafted_files(ctx):
    names = ["deep17_gray", "deep17_444", "deep17_420", "deep18_gray", "zero_runs_gray", "zero_runs_444",
             "long_eob_single"]
    files = [_reference(CRAFTED[n], True) for n in names]
    _decode_and_compare(ctx, files, names, True)


def test_baseline_decoder_reads_the_crafted_files(ctx):
    names = [n for n in CRAFTED if n.split("_")[0] in ("ac", "dc", "zero")]
    files = [_reference(CRAFTED[n], False) for n in names]
    _decode_and_compare(ctx, files, names, False)
