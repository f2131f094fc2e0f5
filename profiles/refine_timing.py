"""Timing of Cloud::refineNormals on the device (gpd_hip_refine_normals) on raw table_mug and the config-4 300k cloud at
k = 10, 30, 50, beside gpd_hip_estimate_normals on the same clouds and the host model (hostlib.refine_normals, one core).
Prints one JSON line: per cloud the points, the estimate_normals wall time (its kernels: a `rocprofv3 --kernel-trace
--stats` run of this script), and per k the passes run and the medians of the call's kernel_ms — the kNN kernel, the
refinement passes launched (device time), the whole call (wall: launches, the copies of the dots and the host's
sequential stop-rule sums between passes, the result's download) — and the host model's wall time.

    python profiles/refine_timing.py [--reps 10] [--host-reps 1]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpd_amd import api, hostlib, synth  # noqa: E402


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()
    ctx = api.Context(api.default_params(15))
    raw = np.load(os.path.join(ROOT, "tests", "golden", "table_mug_xyz.npz"))["xyz"]
    big = synth.make_cloud(1234, 300000, clutter=True)["xyz"]
    out = {"lib": os.path.basename(api.LIB_PATH)}
    for name, xyz in (("table_mug_raw", raw), ("config4_300k", big)):
        ctx.upload_cloud(xyz, np.zeros_like(xyz))
        est = ctx.estimate_normals(0.03)
        row = dict(points=len(xyz), estimate_normals_wall_ms=round(_median_ms(lambda: ctx.estimate_normals(0.03), a.reps), 4))
        for k in (10, 30, 50):
            ms, its = [], 0
            for _ in range(a.reps):
                ctx.upload_cloud(xyz, est)
                its = ctx.refine_normals(k)[1]
                ms.append(ctx.last_refine_ms)
            ms = np.median(np.array(ms), axis=0)
            t0 = time.perf_counter()
            for _ in range(a.host_reps):
                hostlib.refine_normals(xyz, est, k)
            host = (time.perf_counter() - t0) * 1e3 / a.host_reps
            row["k%d" % k] = dict(passes=its, knn_kernel_ms=round(float(ms[0]), 4), passes_kernel_ms=round(float(ms[1]), 4),
                                  call_wall_ms=round(float(ms[2]), 4), host_model_ms=round(host, 1))
        out[name] = row
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
