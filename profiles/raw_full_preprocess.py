#!/usr/bin/env python3
"""What the resident route of a raw scan saves: 16 raw full-flow jobs (tutorials/table_mug's points and a 120k-point synthetic
two-camera scan alternating; voxelise 0.003, normals 0.03, refineNormals(30), sampleAbovePlane, subsample(500)) through
gpd_hip_detect_batch, against the same 16 scans through the single calls — gpd_hip_preprocess_cloud, gpd_hip_upload_cloud,
gpd_hip_estimate_normals, gpd_hip_refine_normals, gpd_hip_sample_above_plane, gpd_hip_detect_select — where every
cloud-sized array crosses PCIe between the steps.  Same process, same context, same weights; two warm-up rounds, then ten
rounds that run the batch and the stepwise route one after the other (so a neighbour on the box disturbs both alike); medians.
Host clock around calls that end in a device synchronise.  The two routes' records are compared byte for byte first.

    python profiles/raw_full_preprocess.py [--out profiles/raw_full_preprocess.json] [--rounds 10] [--jobs 16]
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

from gpd_amd import api, synth  # noqa: E402

CELL, RADIUS, K, DRAWS = 0.003, 0.03, 30, 500
SPREAD = 0.08  # box-to-box and run-to-run spread of a batch figure


def scans():
    mug = np.load(os.path.join(ROOT, "tests", "golden", "table_mug_xyz.npz"))["xyz"].astype(np.float32)
    return [dict(xyz=mug, cam_source=np.ones((1, len(mug)), np.int32), view_points=np.zeros((1, 3))), synth.raw_scan(900, 120000)[0]]


def stepwise(ctx, scan, seed):
    vox, cam, _, _ = ctx.preprocess_cloud(scan["xyz"], scan["cam_source"], None, CELL)
    ctx.upload_cloud(vox, np.zeros_like(vox), cam, scan["view_points"])
    ctx.estimate_normals(RADIUS)  # (also replaces the device copy: the fewest calls a caller of the single entries needs)
    ctx.refine_normals(K)
    above, _, _, _ = ctx.sample_above_plane()
    if len(above):
        si = above[api.sample_positions(len(above), DRAWS, seed, with_repetition=True)]
    else:
        si = api.sample_positions(len(vox), DRAWS, seed, with_repetition=False)
    hands, _, _ = ctx.detect_select(si, 0)
    return hands


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw_full_preprocess.json"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--jobs", type=int, default=16)
    a = ap.parse_args()
    base = scans()
    batch_scans = [base[i % 2] for i in range(a.jobs)]
    seeds = [100 + i for i in range(a.jobs)]
    w = synth.lenet_weights(15, real=dict(np.load(os.path.join(ROOT, "tests", "golden", "lenet15_params.npz"))), trained_magnitude=True)
    ctx = api.Context(api.default_params(15))
    ctx.set_lenet_weights(w)
    jobs, keep = ctx.raw_batch(batch_scans, [None] * a.jobs, None, CELL, RADIUS, refine_normals_k=K, sample_above_plane=True,
                               num_draws=DRAWS, sample_seed=seeds)

    def run_batch():
        t0 = time.perf_counter()
        ctx._check(api.lib().gpd_hip_detect_batch(ctx._h, jobs, len(jobs)))  # returns with every record on the host
        return (time.perf_counter() - t0) * 1e3

    def run_stepwise():
        t0 = time.perf_counter()
        out = [stepwise(ctx, sc, sd) for sc, sd in zip(batch_scans, seeds)]  # every call ends in a device synchronise
        return (time.perf_counter() - t0) * 1e3, out

    # the two routes compute the same thing
    run_batch()
    _, ref = run_stepwise()
    for i, (j, k, r) in enumerate(zip(jobs, keep, ref)):
        assert j.status == 0 and k[5][: j.num_hands].tobytes() == r.tobytes(), "job %d differs from the stepwise route" % i
    for _ in range(max(a.warmup - 1, 0)):
        run_batch()
        run_stepwise()
    tb, ts = [], []
    for _ in range(a.rounds):
        tb.append(run_batch())
        ts.append(run_stepwise()[0])
    mid = jobs[len(jobs) // 2]
    res = {
        "what": "ms per raw scan, full preprocessPointCloud flow (voxelise, normals, refineNormals(30), sampleAbovePlane, 500 draws)",
        "jobs": a.jobs, "rounds": a.rounds, "warmup": a.warmup,
        "points": [int(len(s["xyz"])) for s in base],
        "points_processed": [int(jobs[0].num_points_processed), int(jobs[1].num_points_processed)] if a.jobs > 1 else [int(jobs[0].num_points_processed)],
        "batch_ms_per_scan": statistics.median(tb) / a.jobs,
        "stepwise_ms_per_scan": statistics.median(ts) / a.jobs,
        "batch_ms_per_scan_rounds": [t / a.jobs for t in tb],
        "stepwise_ms_per_scan_rounds": [t / a.jobs for t in ts],
        "middle_job": {"index": len(jobs) // 2, "preprocess_ms": [float(x) for x in mid.preprocess_ms], "host_ms": [float(x) for x in mid.host_ms],
                       "stage_ms": [float(x) for x in mid.stage_ms], "num_candidates": int(mid.num_candidates), "allocs": int(mid.allocs)},
        "spread_allowed": SPREAD,
    }
    res["batch_over_stepwise"] = res["batch_ms_per_scan"] / res["stepwise_ms_per_scan"]
    res["batch_not_slower"] = bool(res["batch_ms_per_scan"] <= res["stepwise_ms_per_scan"] * (1.0 + SPREAD))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    ctx.close()
    if not res["batch_not_slower"]:
        m = res["middle_job"]
        print("the batch route is slower per scan than the stepwise route: preprocess_ms %s, host_ms %s" % (m["preprocess_ms"], m["host_ms"]))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
