#!/usr/bin/env python3
"""Shear rotation throughput (FI_OP_ROTATE_SHEAR, fi_rotate.hip): BASELINE.md's
``r_-45,w_400,h_400`` row against the same batch without ``r_`` -- NIMG
device-resident 1920x1080 sources (seeded synthetic pool), one
fi_process_batch_device per pass, REPS alternating passes of the two option
strings after a warm-up of each; median and min-max images/s of both.  One more
timed pass (fi_set_timing) reads the rotation stage's kernel time from
fi_kernel_stats("rotate") and sets it against its algorithmic bytes (the Q16
image in, the 8-bit image out) at 8 TB/s.  Prints one JSON line and writes it to
profiles/rotate/rotate_bench.json.  A sheared image leaves the streaming MFMA
resample kernels for the generic two-pass ones (they write the Q16 image the
stage reads), so the comparison measures that as well."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flyimg_amd import _lib as L  # noqa: E402
from flyimg_amd.processor import ImageProcessor, OptionsBag  # noqa: E402
from flyimg_amd.runtime import Context, _fill  # noqa: E402

N = int(os.environ.get("NIMG", "256"))
W, H = 1920, 1080
REPS = int(os.environ.get("REPS", "7"))
WARMUP = int(os.environ.get("WARMUP", "2"))
ARMS = {"rotate": "w_400,h_400,r_-45", "plain": "w_400,h_400"}
HBM_BYTES_PER_S = 8e12


def main():
    with Context(0) as ctx:
        stride = W * 3
        pool = ctx.malloc(stride * H * N)
        for i in range(N):
            ctx.fill_synthetic(pool + i * stride * H, W, H, stride, 100 + i)
        arrs, bases = {}, []
        for arm, options in ARMS.items():
            op = ImageProcessor(OptionsBag(options), W, H, shear_rotate=True).to_op()
            arr = (L.FiImage * N)()
            for i in range(N):
                a = arr[i]
                a.src, a.src_w, a.src_h, a.src_stride, a.src_channels = pool + i * stride * H, W, H, stride, 3
                _fill(a, op)
            L.check(L.lib().fi_plan(arr, N))
            cap = (arr[0].out_stride * arr[0].out_h + 255) // 256 * 256
            base = ctx.malloc(cap * N)
            bases.append(base)
            for i in range(N):
                arr[i].dst, arr[i].dst_capacity = base + i * cap, cap
            arrs[arm] = arr

        def one(arm):
            t0 = time.perf_counter()
            L.check(ctx.process_device(arrs[arm], N))
            return time.perf_counter() - t0

        for _ in range(WARMUP):
            for arm in ARMS:
                one(arm)
        ts = {arm: [] for arm in ARMS}
        for _ in range(REPS):  # alternating: both arms see the same machine state
            for arm in ARMS:
                ts[arm].append(one(arm))
        ctx.set_timing(True)
        ctx.reset_stats()
        one("rotate")
        k_ms, launches, k_bytes = ctx.stats("rotate")
        rs_ms = ctx.stats("resize")[0]
        ctx.reset_stats()
        one("plain")
        rs_plain_ms = ctx.stats("resize")[0]
        ctx.set_timing(False)
        out = arrs["rotate"][0]
        px = ctx.d2h(out.dst, out.out_stride * out.out_h).reshape(out.out_h, out.out_w, 3)
        assert (px[0, 0] == 255).all() and px[out.out_h // 2, out.out_w // 2].min() < 255  # white corners, image inside
        for b in bases:
            ctx.free(b)
        ctx.free(pool)

    def ips(t):
        return {"median": round(N / float(np.median(t)), 1), "min": round(N / max(t), 1), "max": round(N / min(t), 1)}

    floor_ms = k_bytes / HBM_BYTES_PER_S * 1e3
    res = {
        "images": N, "source": f"{W}x{H}", "passes": REPS, "warmup": WARMUP,
        "rotate_options": ARMS["rotate"], "rotate_out": f"{out.out_w}x{out.out_h}",
        "rotate_images_per_s": ips(ts["rotate"]),
        "plain_options": ARMS["plain"], "plain_images_per_s": ips(ts["plain"]),
        "k_rotate_ms": round(k_ms, 3), "k_rotate_launches": int(launches), "k_rotate_bytes": int(k_bytes),
        "k_rotate_ms_at_8TBps": round(floor_ms, 4), "k_rotate_over_floor": round(k_ms / floor_ms, 1) if floor_ms else None,
        "resize_stage_ms_rotate": round(rs_ms, 3), "resize_stage_ms_plain": round(rs_plain_ms, 3),
    }
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles", "rotate"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "rotate", "rotate_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
