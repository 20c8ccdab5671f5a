"""Change detector for the files the GPU PNG and lossless WebP encoders write.

Context.png_encode and Context.webp_encode (through their _host forms,
which upload the arrays first) encode the cases of
tests/_enc_digest_cases.py, one batched call per format; the length and
SHA-256 of every file are compared with tests/golden/enc_digests.json.  The
WebP entries are the ones tests/test_enc_digest_cpu.py holds the host form to
(the device's file is the host form's); the PNG entries were recorded from the
device, which has no host form.

This pins bytes, not correctness -- tests/test_gpu_png_encode.py,
tests/test_gpu_webp_encode.py and tests/test_gpu_lossless_content.py decode
what is written.  A change that alters the encoders' output on purpose
re-records the file (the failure message prints the new values) and says so in
its description.
"""
import pytest

from flyimg_amd.runtime import Context

from . import _enc_digest_cases as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _digests(cases, files):
    assert all(f is not None for f in files), [c.name for c, f in zip(cases, files) if f is None]
    return {c.name: D.digest(f) for c, f in zip(cases, files)}


def test_png_files_are_unchanged(ctx):
    cases = D.png_cases()
    files = ctx.png_encode_host([c.px for c in cases], [c.param for c in cases])
    D.compare("png", _digests(cases, files))


def test_webp_files_are_unchanged(ctx):
    cases = D.webp_cases()
    files = ctx.webp_encode_host([c.px for c in cases], [c.param for c in cases])
    D.compare("webp", _digests(cases, files))
