#!/usr/bin/env python
"""One view of training-set generation, two routes, alternating in one process:

  resident  Context.label_view: the ground truth uploaded once, rounds / accumulator / selection on the device, one copy back
  composed  the public calls that existed before it, per round: upload_cloud(view), search, workspace filter on the host,
            images with download, upload_cloud(ground truth), reevaluate; then the balance on the host

on the size a user would run: the 30 000-point scene, a ground truth of 60 000 points, three rounds of 400 samples, C = 15,
max_grasps_per_view = 500.  Host clock around each route (both end in a synchronise), median and spread of REPEATS runs after
a warm-up.  The two routes must return the same bytes.   python profiles/label_view_ab.py [out.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402  (the host workspace filter of the composed route)
from gpd_amd import api, synth  # noqa: E402

REPEATS, WARMUP, ROUNDS, SAMPLES, MAX_GRASPS, CHANNELS = 24, 3, 3, 400, 500, 15
HAND = api.HAND_DTYPE.itemsize


def main():
    cl = synth.make_cloud(1234, 30000)
    rng = np.random.RandomState(5)
    gt = np.concatenate([cl["xyz"], (cl["xyz"] + rng.uniform(-0.0003, 0.0003, cl["xyz"].shape)).astype(np.float32)])
    gn = np.concatenate([cl["normals"]] * 2)
    obj = np.flatnonzero(cl["is_object"])
    rounds = np.stack([np.random.RandomState(70 + r).choice(obj, SAMPLES, replace=False) for r in range(ROUNDS)]).astype(np.int32)
    op = oracle.default_params(CHANNELS)
    ctx = api.Context(api.default_params(CHANNELS))
    slots = ctx.n_slots

    def resident():
        return ctx.label_view(rounds, 10 ** 6, MAX_GRASPS)

    def composed():
        imgs, recs, labs, d2h = [], [], [], 0
        for r in range(ROUNDS):
            ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
            hands = oracle.filter_workspace(op, ctx.search(rounds[r]))
            img, cand = ctx.images(hands)
            cr = hands.reshape(-1)[cand]
            ctx.upload_cloud(gt, gn)
            lab, cr = ctx.reevaluate(cr)
            imgs.append(img)
            recs.append(cr)
            labs.append(lab.astype(np.uint8))
            # what these calls copy device -> host: every record of the search and its neighbourhood counts, every image and its
            # candidate index, the re-evaluated records and their labels
            d2h += SAMPLES * slots * HAND + SAMPLES * 32 + img.nbytes + cand.nbytes + len(cr) * HAND + lab.nbytes
        lab = np.concatenate(labs)
        keep = api.balance_view(lab, MAX_GRASPS)
        return dict(images=np.concatenate(imgs)[keep], hands=np.concatenate(recs)[keep], labels=lab[keep], d2h_bytes=d2h,
                    num_candidates=len(lab), num_positives=int(lab.sum()))

    ctx.upload_ground_truth(gt, gn)
    ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
    a, b = resident(), composed()
    same = all(a[k].tobytes() == b[k].tobytes() for k in ("images", "hands", "labels"))
    assert same and a["num_candidates"] == b["num_candidates"], "the two routes disagree"
    times = {"resident": [], "composed": []}
    stage = []
    for i in range(WARMUP + REPEATS):
        for name, fn in (("resident", resident), ("composed", composed)):
            if name == "resident":  # the view the composed route left is the ground truth: a view's own upload is part of neither
                ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
            t0 = time.perf_counter()
            out = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= WARMUP:
                times[name].append(dt)
                if name == "resident":
                    stage.append(out["stage_ms"])
    res = dict(view_points=30000, ground_truth_points=len(gt), rounds=ROUNDS, samples_per_round=SAMPLES, channels=CHANNELS,
               max_grasps_per_view=MAX_GRASPS, repeats=REPEATS, num_candidates=a["num_candidates"], num_positives=a["num_positives"],
               num_out=a["num_out"], gt_neighbourhoods=a["gt_neighbourhoods"], same_bytes=bool(same))
    for name in times:
        t = np.array(times[name])
        res[name + "_ms"] = dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()), p25=float(np.percentile(t, 25)),
                                 p75=float(np.percentile(t, 75)))
    res["resident_stage_ms_median"] = dict(zip(("search", "images", "labels", "select_gather"), np.median(np.array(stage), axis=0).tolist()))
    res["d2h_bytes"] = dict(resident=int(a["d2h_bytes"]), composed=int(b["d2h_bytes"]))
    res["speedup_median"] = res["composed_ms"]["median"] / res["resident_ms"]["median"]
    ctx.close()
    line = json.dumps(res, indent=1)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
