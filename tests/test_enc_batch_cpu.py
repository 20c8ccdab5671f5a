"""The host helpers the four GPU encoders' batch functions share
(flyimg_amd/csrc/fi_enc_batch.h), no GPU: tests/native/enc_batch_driver.cpp
includes the header alone and is built with the system C++ compiler -- no HIP
header, nothing of the library -- under ASan/UBSan, run in its own process with
nothing preloaded.  The cases: the arena offsets against a hand-written
up256 ladder, the per-image argument check, and enc_deliver at len == cap, at
len == cap + 1 with and without the prefix copy, at cap == 0 with a null
buffer, and around images rejected in the middle of a batch."""
import os
import shutil
import subprocess
import tempfile

import pytest

from .test_sanitize_cpu import ENV, ROOT, SAN

CASES = ["arena", "io_status", "deliver_len_eq_cap", "deliver_short_prefix", "deliver_short_no_prefix",
         "deliver_cap0_null", "deliver_rejected_middle"]


@pytest.fixture(scope="module")
def results():
    cxx = shutil.which("c++") or shutil.which("g++")
    if not cxx:
        pytest.skip("no system C++ compiler")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "enc_batch")
        subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *SAN,
                        os.path.join(ROOT, "tests/native/enc_batch_driver.cpp"), "-o", exe],
                       check=True, capture_output=True, timeout=300)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert "DONE" in lines
    return {ln.split()[1].rstrip(":"): ln for ln in lines if ln.startswith(("PASS ", "FAIL "))}


def test_driver_runs_every_case(results):
    assert sorted(results) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_enc_batch(results, case):
    assert results[case] == f"PASS {case}", results[case]
