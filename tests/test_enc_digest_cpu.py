"""Change detector for the bytes the lossless encoders' host code writes (no
GPU).

The lossless WebP host form (fi_debug_webp_encode_host: the inline code the
device runs, so its file is the device's) encodes the cases of
tests/_enc_digest_cases.py, and tests/native/png_write_driver.cpp answers the
`huff` and `block` inputs of tests/test_png_encode_cpu.py.  The length and
SHA-256 of every file and of every answer line are compared with
tests/golden/enc_digests.json: the prefix-code builder's tie order, the
code-length run-length coder and the bit writers are all in those bytes, so a
refactor that moves one of them fails here, on the CPU.

This pins bytes, not correctness -- tests/test_webp_encode_cpu.py,
tests/test_lossless_content_cpu.py and tests/test_png_encode_cpu.py decode
what is written.  A change that alters the encoders' output on purpose
re-records the file (the failure message prints the new values) and says so in
its description.
"""
from flyimg_amd.runtime import webp_encode_host_form

from . import _enc_digest_cases as D
from .test_png_encode_cpu import _block_lines, _huff_lines, driver  # noqa: F401  (driver: the fixture)


def test_webp_host_form_bytes_are_unchanged():
    D.compare("webp", {c.name: D.digest(webp_encode_host_form(c.px, c.param)) for c in D.webp_cases()})


def test_png_code_builder_answers_are_unchanged(driver):  # noqa: F811
    lines = _huff_lines() + _block_lines(1) + _block_lines(0)
    names = [f"huff_{k}" for k in range(len(_huff_lines()))]
    names += [f"block_last{last}_{k}" for last in (1, 0) for k in range(len(_block_lines(last)))]
    out = driver(lines)
    D.compare("png_driver", {n: D.digest(line.encode()) for n, line in zip(names, out)})
