#!/usr/bin/env python
"""The cost of the shadow jitter (gpd_hip_set_shadow_jitter) and of carrying it, into profiles/shadow_jitter_ab.json.

  default path   `python bench.py --gpus 1` of the parent commit and of this tree, interleaved on one GPU, N runs each: the JSON
                 lines of the two series are handed in as files (--parent-lines, --change-lines).  The image-stage time of a
                 line is kernels.grasp_image_kernel.ms; jitter is off there, and the default instantiations are the parent's
                 instruction for instruction, so this tree's median has to lie inside the spread of the parent's own runs.
  jitter on      the same candidate list (bench.py's configuration 2: the 30 000-point scene, the first 5000 valid candidates
                 after the workspace filter, 15 channels) through Context: the image stage re-launched on the resident list
                 (gpd_hip_replay, stage 1; HIP events around the stage), jitter off and on alternating, and the window class
                 each setting ran.  Run it with GPD_HIP_LIB pointing at the profiling build.

   python profiles/shadow_jitter_ab.py --parent-lines A.jsonl --change-lines B.jsonl [--out profiles/shadow_jitter_ab.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (its workspace filter: the benchmark's own candidate list)
from gpd_amd import api, synth  # noqa: E402

POINTS, CANDIDATES, CHANNELS, STEPS, WARMUP, ROUNDS, SEED = 30000, 5000, 15, 20, 3, 5, 2026


def image_ms_of(path):
    out = []
    for line in open(path):
        line = line.strip()
        if line.startswith("{"):
            out.append(float(json.loads(line)["kernels"]["grasp_image_kernel"]["ms"]))
    return out


def series(ms):
    return dict(image_stage_ms=ms, median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms))) if ms else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lines")
    ap.add_argument("--change-lines")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shadow_jitter_ab.json"))
    args = ap.parse_args()
    cl = synth.make_cloud(1234, POINTS)
    ctx = api.Context(api.default_params(CHANNELS))
    ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
    si = synth.sample_indices(cl, min(CANDIDATES // 2 + 64, int(cl["is_object"].sum())))
    hands = ctx.search(si).copy()
    bench._filter_workspace(hands, ctx.params)
    flat = hands.reshape(-1)
    vidx = np.flatnonzero(flat["valid"])
    flat["valid"][vidx[CANDIDATES:]] = 0
    res = {0: dict(ms=[]), 1: dict(ms=[])}
    for rnd in range(ROUNDS):
        for on in (0, 1):
            ctx.set_shadow_jitter(on, SEED)
            _, cand = ctx.images(hands, download=False)
            route, info = ctx.image_routes()
            assert info["status"] == 0 and len(cand) == CANDIDATES
            res[on].update(window_class=info["window_class"], large_shadow_instantiation=int((route & 1).sum()),
                           general_kernel=int((route & 2).sum()), large_points_kernel=int((route & 4).sum()))
            for _ in range(WARMUP):
                ctx.replay(1)
            ctx.replay_times()
            for _ in range(STEPS):
                ctx.replay(1)
            img_ms, _, launches, _ = ctx.replay_times()
            assert launches == STEPS
            res[on]["ms"].append(img_ms / STEPS)
    ctx.close()
    out = dict(
        workload="bench.py configuration 2: %d points, %d candidates, %d channels; image stage alone" % (POINTS, CANDIDATES, CHANNELS),
        library=os.path.basename(api.LIB_PATH),
        bench_default_path=dict(parent=series(image_ms_of(args.parent_lines)) if args.parent_lines else None,
                                change=series(image_ms_of(args.change_lines)) if args.change_lines else None),
        context_replay={("jitter_on" if on else "jitter_off"): dict(series(r.pop("ms")), **r) for on, r in res.items()})
    b = out["bench_default_path"]
    if b["parent"] and b["change"]:
        b["change_median_inside_parent_spread"] = bool(b["parent"]["min"] <= b["change"]["median"] <= b["parent"]["max"])
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
