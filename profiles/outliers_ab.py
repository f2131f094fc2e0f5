#!/usr/bin/env python3
"""What removeStatisticalOutliers costs (mean_k 50, multiplier 1.0, the reference's values).

On the 120k-point synthetic two-camera scan of profiles/raw_full_preprocess.py, voxelised at 0.003:
  - gpd_hip_remove_statistical_outliers on the uploaded cloud: device ms of the distance kernel and of the compaction
    (HIP events) and host ms of the whole call (it ends in a device synchronise); three warm-up calls, then medians of 20;
  - the host model (gpd_amd/csrc/outlier_model.h) on one core, median of 3.
Then the raw batch route of profiles/raw_full_preprocess.py — 16 raw full-flow jobs, tutorials/table_mug's points and that scan
alternating; voxelise, normals, refineNormals(30), sampleAbovePlane, subsample(500) — with the step on and off: two warm-up
rounds, then ten rounds that run the two batches one after the other (a neighbour on the box disturbs both alike); medians,
ms per scan.  The step-off figure is the one profiles/raw_full_preprocess.json holds from the parent commit, quoted beside it.

    python profiles/outliers_ab.py [--out profiles/outliers_ab.json] [--rounds 10] [--jobs 16]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gpd_amd import api, hostlib, synth  # noqa: E402

CELL, RADIUS, K, DRAWS = 0.003, 0.03, 30, 500
MEAN_K, MULT = 50, 1.0


def scans():
    mug = np.load(os.path.join(ROOT, "tests", "golden", "table_mug_xyz.npz"))["xyz"].astype(np.float32)
    return [dict(xyz=mug, cam_source=np.ones((1, len(mug)), np.int32), view_points=np.zeros((1, 3))), synth.raw_scan(900, 120000)[0]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outliers_ab.json"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    base = scans()
    w = synth.lenet_weights(15, real=dict(np.load(os.path.join(ROOT, "tests", "golden", "lenet15_params.npz"))), trained_magnitude=True)
    ctx = api.Context(api.default_params(15))
    ctx.set_lenet_weights(w)

    # the single call
    scan = base[1]
    vox, cam, _, _ = ctx.preprocess_cloud(scan["xyz"], scan["cam_source"], None, CELL)
    zeros = np.zeros_like(vox)
    ms = []
    for i in range(3 + a.calls):
        ctx.upload_cloud(vox, zeros, cam, scan["view_points"])
        kept, stats, _ = ctx.remove_statistical_outliers(MEAN_K, MULT)
        if i >= 3:
            ms.append(ctx.last_outlier_ms)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        hk, hs, _ = hostlib.remove_statistical_outliers(vox, MEAN_K, MULT)
        host.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(hk, kept) and hs.tobytes() == stats.tobytes(), "the device differs from the host model"

    # the raw batch route, step on and off
    batch_scans = [base[i % 2] for i in range(a.jobs)]
    seeds = [100 + i for i in range(a.jobs)]
    common = dict(refine_normals_k=K, sample_above_plane=True, num_draws=DRAWS, sample_seed=seeds)
    off, _keep_off = ctx.raw_batch(batch_scans, [None] * a.jobs, None, CELL, RADIUS, **common)
    on, _keep_on = ctx.raw_batch(batch_scans, [None] * a.jobs, None, CELL, RADIUS, outlier_mean_k=MEAN_K, outlier_stddev_mult=MULT, **common)

    def run(jobs):
        t0 = time.perf_counter()
        ctx._check(api.lib().gpd_hip_detect_batch(ctx._h, jobs, len(jobs)))  # returns with every record on the host
        return (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        run(off)
        run(on)
    t_off, t_on = [], []
    for _ in range(a.rounds):
        t_off.append(run(off))
        t_on.append(run(on))
    assert all(j.status == 0 for j in on) and all(j.status == 0 for j in off)
    with open(os.path.join(ROOT, "profiles", "raw_full_preprocess.json")) as f:
        parent = json.load(f)
    res = {
        "what": "removeStatisticalOutliers(50, 1.0): the single call on the voxelised 120k-point scan, and ms per raw scan of the full "
                "preprocessPointCloud batch flow with the step on and off",
        "points": int(len(vox)), "kept": int(len(kept)), "mean_stddev_threshold": [float(x) for x in stats],
        "calls": a.calls,
        "distance_kernel_ms": statistics.median(m[0] for m in ms),
        "compaction_ms": statistics.median(m[1] for m in ms),
        "whole_call_ms": statistics.median(m[2] for m in ms),
        "host_model_one_core_ms": statistics.median(host),
        "jobs": a.jobs, "rounds": a.rounds, "warmup": a.warmup,
        "batch_points_processed_off": [int(off[0].num_points_processed), int(off[1].num_points_processed)] if a.jobs > 1 else [],
        "batch_points_processed_on": [int(on[0].num_points_processed), int(on[1].num_points_processed)] if a.jobs > 1 else [],
        "batch_outlier_ms_on": [float(on[0].outlier_ms), float(on[1].outlier_ms)] if a.jobs > 1 else [],
        "batch_ms_per_scan_off": statistics.median(t_off) / a.jobs,
        "batch_ms_per_scan_on": statistics.median(t_on) / a.jobs,
        "batch_ms_per_scan_off_rounds": [t / a.jobs for t in t_off],
        "batch_ms_per_scan_on_rounds": [t / a.jobs for t in t_on],
        "parent_batch_ms_per_scan": parent["batch_ms_per_scan"],  # profiles/raw_full_preprocess.json, measured on the parent commit
    }
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
