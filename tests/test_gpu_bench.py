"""bench.py end to end on the GPU at a small batch: what a plain run prints and
leaves out, what --full adds, and that --dump-outputs writes the same arrays
from both (same arguments, same seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--images", "16"]


def _bench(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "FI_RDZV_ID")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + extra, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_and_full_runs_and_their_dumps(tmp_path):
    plain = _bench(["--dump-outputs", str(tmp_path / "plain")])
    full = _bench(["--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")])
    for d in (plain, full):
        assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "Mpix/s" and d["dtype"] == "u8"
        assert d["higher_is_better"] is True and d["failed_images"] == 0
        assert d["ms_per_step"] > 0
        # value and ms_per_step are the same measurement: 16 images of 1920x1080 per step
        # (ms_per_step is rounded to 1e-4 ms; a step of >= 0.02 ms keeps that within 0.5 %)
        assert d["ms_per_step"] >= 0.02
        assert d["value"] == pytest.approx(16 * 1920 * 1080 / 1e6 / (d["ms_per_step"] / 1e3), rel=1e-2)
    # a plain run leaves out the oracle check, the stage pass and the CPU baseline
    assert plain["verified"].startswith("skipped") and "cpu_baseline" not in plain
    assert all(k.startswith("host_") for k in plain["stages_ms_per_step"])
    ok, total = full["verified"].split(" ")[0].split("/")  # "<ok>/<checked> images of the last timed batch ..."
    assert ok == total and int(total) > 0 and "resize" in full["stages_ms_per_step"]
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == ["pixel_index.npy", "pixels.npy", "records.npy"] == sorted(os.listdir(tmp_path / "full"))
    a = {n: np.load(tmp_path / "plain" / n) for n in names}
    assert all(np.array_equal(a[n], np.load(tmp_path / "full" / n)) for n in names)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["pixels.npy"].dtype == np.float32 and a["records.npy"].dtype == np.float64
    rec = a["records.npy"]
    assert rec.shape[0] == 16 and list(rec[:, 0]) == list(range(16)) and not rec[:, 1].any()  # every status 0
    # w_500,smc_1: each image's pixels are its applied crop box of the 500x281 resize
    w, h, c = (rec[:, 1 + i] for i in (1, 2, 3))
    assert (w <= 500).all() and (h <= 281).all() and (c == 3).all()
    idx = a["pixel_index.npy"].astype(int)
    assert len(idx) == 16 and a["pixels.npy"].size == int((w * h * c).sum())
    assert a["pixels.npy"].min() >= 0 and a["pixels.npy"].max() <= 255 and a["pixels.npy"].std() > 1
