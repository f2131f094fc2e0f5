#!/usr/bin/env python
"""Host-clock timings of two entries the benchmark has no repeated leg for: Context.label_view (the resident route of
profiles/label_view_ab.py: 30k-point view, 60k-point ground truth, three rounds of 400 samples) and Context.estimate_normals on
the benchmark's 30k-point cloud.  Median / min / max of REPEATS calls after a warm-up, one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpd_amd import api, synth  # noqa: E402

REPEATS, WARMUP = 15, 3


def stats(ts):
    t = np.array(ts)
    return dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()))


def main():
    cl = synth.make_cloud(1234, 30000)
    rng = np.random.RandomState(5)
    gt = np.concatenate([cl["xyz"], (cl["xyz"] + rng.uniform(-0.0003, 0.0003, cl["xyz"].shape)).astype(np.float32)])
    gn = np.concatenate([cl["normals"]] * 2)
    obj = np.flatnonzero(cl["is_object"])
    rounds = np.stack([np.random.RandomState(70 + r).choice(obj, 400, replace=False) for r in range(3)]).astype(np.int32)
    ctx = api.Context(api.default_params(15))
    ctx.upload_ground_truth(gt, gn)
    ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
    lv = []
    for i in range(WARMUP + REPEATS):
        t0 = time.perf_counter()
        out = ctx.label_view(rounds, 10 ** 6, 500)
        if i >= WARMUP:
            lv.append((time.perf_counter() - t0) * 1e3)
    grid = synth.make_cloud(4321, 30000)
    ctx.upload_cloud(grid["xyz"], np.zeros_like(grid["xyz"]), grid["cam_source"], grid["view_points"])
    nm = []
    for i in range(WARMUP + REPEATS):
        t0 = time.perf_counter()
        ctx.estimate_normals(0.03)
        if i >= WARMUP:
            nm.append((time.perf_counter() - t0) * 1e3)
    ctx.close()
    print(json.dumps(dict(lib=os.environ.get("GPD_HIP_LIB", "tree"), label_view_ms=stats(lv), label_view_candidates=int(out["num_candidates"]),
                          estimate_normals_ms=stats(nm))))


if __name__ == "__main__":
    main()
