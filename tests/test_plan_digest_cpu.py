"""Change detector for the host planner's output (no GPU).

fi_debug_host_plan plans a fixed sequence of small batches on one host-only
context -- later batches see the earlier ones' cached tables and heap offsets,
as in serving -- and (NULL, 3, 0, ms) reports a 64-bit FNV-1a digest of each
packed upload blob with the workspace size, the blob's bytes and the tile and
smartcrop counts.  They are compared with tests/golden/plan_digests.json: every
descriptor field, tile order and heap offset is in those bytes, so a refactor
of the planner that moves one of them fails here, on the CPU, before any pixel
test runs.

test_planner_tables_are_unchanged does the same one level down: it compiles
tests/native/plan_driver.cpp with the planner's sources alone and compares the
digest of every structure fi_plan.h's builders fill -- each scalar field and
vector of ImPlan, the tap axes, the quantised weights, the MFMA tables of the
three resample kernels, ScPlan with its fragment tables, the importance and
score tables -- on tests/_planner.py plan_lines(), one digest per builder per
input line so that a mismatch names the builder.

This pins bytes, not correctness.  A change that alters the planner's output on
purpose re-records the file (the failure message prints the new values) and
says so in its description.
"""
import ctypes
import json
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import bench
from flyimg_amd import _lib as L
from tests._planner import PLANNER_SRCS, ROOT, plan_lines
from tests.test_plan_cpu import _batch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "plan_digests.json")
FIELDS = ("digest", "blob", "vtiles", "vrtiles", "htiles", "sc")


def _sequence():
    cfg4 = [(W, H, bench.CFG4_OPS[k]) for W, H, k in bench.cfg4_list(65536)[:256]]
    return [
        ("cfg2", [(1920, 1080, "w_500,smc_1")] * 64, 16),
        ("crop_4k", [(3840, 2160, "w_512,h_512,c_1")] * 32, 16),
        # Q16 tiles, rotation, the gray smartcrop route
        ("gray_rot_smc", [(6000, 4000, "w_400,h_400,c_1,r_90,clsp_Gray,smc_1")] * 32, 16),
        # >= 2048 strips: whole-image tiles, no bands
        ("whole_image", [(3000, 2000, "w_300,h_250,c_1")] * 2100, 16),
        # mixed classes: the seam drop, the nocb split, LPT
        ("cfg4", cfg4, 16),
        ("cfg4_cached", cfg4, 16),
        ("upscales", [(200, 150, "w_640"), (64, 48, "w_300,h_300,c_1"), (333, 777, "h_100,r_270")], 16),
        ("mono_conv", [(800, 600, "w_200,h_200,c_1,mnchr_1"), (800, 600, "w_200,blr_1"), (1200, 900, "w_300,sh_1")], 16),
        # xf > yf after rounding: ImPlan::hfirst, k_rs_hv
        ("hfirst", [(1001, 3000, "w_333")] * 4 + [(1920, 1080, "w_500")] * 2, 16),
        # rows at a 4-byte pitch: no 16-byte loads, the generic modes 0-2
        ("unaligned", [(1921, 1080, "w_500"), (1001, 3000, "w_333"), (640, 480, "r_90")], 4),
    ]


def _plan_all(lib):
    out = []
    try:
        for name, items, align in _sequence():
            arr = _batch(items, align)
            ms = (ctypes.c_double * 7)()
            L.check(lib.fi_debug_host_plan(arr, len(arr), 1, ms))
            r = (ctypes.c_double * 7)()
            L.check(lib.fi_debug_host_plan(None, 3, 0, r))
            out.append({"name": name, "digest": "%08x%08x" % (int(r[1]), int(r[0])), "blob": int(r[2]),
                        "vtiles": int(r[3]), "vrtiles": int(r[4]), "htiles": int(r[5]), "sc": int(r[6])})
    finally:
        lib.fi_debug_host_plan(None, 0, 0, None)  # the next run's context reads FI_VR_RS again
    return out


@pytest.mark.parametrize("vr_rs", [None, "0"], ids=["vr", "vm"])
def test_planner_output_is_unchanged(vr_rs, monkeypatch):
    """The digests of the sequence, with FI_VR_RS unset and with FI_VR_RS=0,
    equal the recorded ones (see the module docstring: a change detector)."""
    lib = L.lib()
    lib.fi_debug_host_plan(None, 0, 0, None)
    if vr_rs is None:
        monkeypatch.delenv("FI_VR_RS", raising=False)
    else:
        monkeypatch.setenv("FI_VR_RS", vr_rs)
    got = _plan_all(lib)
    by = {g["name"]: g for g in got}
    # the sequence reaches every tile builder and the generic path (by the
    # counts the hook reports, not by assumption)
    assert by["hfirst"]["htiles"] > 0, by["hfirst"]
    assert by["unaligned"]["vtiles"] == by["unaligned"]["vrtiles"] == by["unaligned"]["htiles"] == 0, by["unaligned"]
    assert by["cfg2"]["sc"] == 64 and by["gray_rot_smc"]["sc"] == 32
    if vr_rs is None:
        assert any(g["vtiles"] > 0 and g["vrtiles"] > 0 for g in got), got
        assert by["whole_image"]["vrtiles"] >= 2048, by["whole_image"]
    else:
        assert all(g["vrtiles"] == 0 for g in got), got
        assert by["cfg2"]["vtiles"] > 0
    with open(GOLDEN) as f:
        want = json.load(f)["vr" if vr_rs is None else "vm"]
    diff = [(w, g) for w, g in zip(want, got) if any(w[k] != g[k] for k in ("name",) + FIELDS)]
    assert len(want) == len(got) and not diff, (
        "the planner's output changed; first difference (recorded, now): %r\nnew values:\n%s"
        % (diff[:1], json.dumps(got, indent=1)))


# every table variant a fragment writer of the planner can take (plan_driver's
# DONE line: name=count), and the builders (name=built/refused)
VARIANTS = ("plan_im.gray", "plan_im.shear", "axis.outputs_not_16n", "mfma_h.frag2", "mfma_h.ks2", "mfma_h.frag2_ks2",
            "vm_v.rstep0", "vr_v.ks2", "vr_v.rstep0", "hv_h.ks2", "hv_v.ks2", "sc.hm", "sc.hm_ks2", "sc.vq", "sc.cx",
            "sc.cx_kv2", "sc.fz", "sc.reduce", "sc.hm_not_vq", "importance.wider_than_64", "score_btab.ks1",
            "score_btab.ks2")
BUILDERS = ("plan_im", "axis_v", "axis_h", "vr_quant_v", "vr_quant_h", "axis_q22_v", "axis_q22_h", "mfma_h168",
            "mfma_h64", "mfma_h48", "mfma_h32", "vm_v", "vr_v", "hv_h", "hv_v", "plan_sc", "importance_image",
            "importance_window", "score_btab1", "score_btab2", "score_btab3", "score_btab_image")


def test_planner_tables_are_unchanged():
    """Every builder's digest on every input line equals the recorded one, and
    the inputs reach every builder and every table variant at least once."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    lines = plan_lines()
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "plan_driver")
        subprocess.run([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests/native/plan_driver.cpp"), *PLANNER_SRCS, "-o", exe],
                       check=True, capture_output=True, timeout=300)
        stdin = "".join(" ".join(str(int(v)) for v in ln) + "\n" for ln in lines)
        r = subprocess.run([exe], input=stdin, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    got = r.stdout.splitlines()
    assert got and got[-1].startswith(f"DONE {len(lines)} images;"), got[-1:]
    done = dict(kv.split("=") for kv in got[-1].split(";")[1].split())
    for b in BUILDERS:
        assert int(done[b].split("/")[0]) > 0, (b, done[b])
    for v in VARIANTS:
        assert int(done[v]) > 0, (v, done[v])
    assert set(done) == set(BUILDERS) | set(VARIANTS), sorted(set(done) ^ (set(BUILDERS) | set(VARIANTS)))
    with open(GOLDEN) as f:
        want = json.load(f)["tables"]
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert len(want) == len(got) and not diff, (
        "the planner's tables changed; first differences (recorded, now): %r; builders that differ: %s"
        % (diff[:3], sorted({re.split(" ", g)[1] for _, g in diff})))
