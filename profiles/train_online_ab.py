#!/usr/bin/env python
"""Filling a trainer's two resident sets from labelled views, two routes, alternating passes in one process:

  A  files' route without the files: Context.label_view per view (the kept set is copied to the host), concatenation and the
     per-object shuffle on the host, Trainer.set_data of both sets at the end
  B  Trainer.append_view per view (the kept set is gathered into the pool on the device), Trainer.reorder per object

on the synthetic data set of tests/test_gpu_generate_data.py: two objects x three views, C = 3, 12 samples per round.  The
views are preprocessed once (voxel grid, normals) and their upload is part of neither route; both routes start from empty
sets in every pass, so B's pools grow as they would for a user who reserved nothing.  Host clock around each call (every call
ends in a synchronise); a pass's time over its six views is the per-view figure.  WARMUP passes of each route, then REPEATS;
median and min - max.  Both routes must leave the same bytes in the sets.   python profiles/train_online_ab.py [out.json]
"""
import json
import os
import pathlib
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_generate_data as gd  # noqa: E402  (the data set and its settings)
from gpd_amd import api  # noqa: E402

REPEATS, WARMUP = 20, 3


def main():
    with tempfile.TemporaryDirectory() as tmp:
        _, _, clouds = gd._data_set(pathlib.Path(tmp))
    C = gd.CHANNELS
    ctx = api.Context(api.default_params(C))
    trainer = api.Trainer(ctx)
    objects = []
    for o, name in enumerate(gd.OBJECTS):
        mesh, views = clouds[name]
        ctx.upload_cloud(mesh, np.zeros_like(mesh))
        gt_normals = -ctx.estimate_normals(gd.RADIUS)
        prepared = []
        for j, v in enumerate(views):
            xyz, cam, _, _ = ctx.preprocess_cloud(v, np.ones((1, len(v)), np.int32), None, gd.VOXEL)
            ctx.upload_cloud(xyz, np.zeros_like(xyz), cam, np.zeros((1, 3)))
            normals = -ctx.estimate_normals(gd.RADIUS)
            seed = (gd.SAMPLE_SEED + 1000003 * (o * gd.VIEWS + j)) & 0xFFFFFFFF
            rounds = np.stack([api.sample_positions(len(xyz), gd.NUM_SAMPLES, (seed + r) & 0xFFFFFFFF) for r in range(gd.MAX_ROUNDS)])
            prepared.append((xyz, normals, cam, rounds, 1 if j in gd.TEST_VIEWS else 0))
        objects.append((mesh, gt_normals, prepared))
    num_views = sum(len(p) for _, _, p in objects)
    empty = (np.zeros((0, 60, 60, C), np.uint8), np.zeros(0, np.uint8))

    def one_pass(route):
        """-> (ms inside the route's calls, bytes device -> host, bytes host -> device, the view calls' results)"""
        ms, d2h, h2d, outs = 0.0, 0, 0, []
        for which in (0, 1):
            trainer.set_data(*empty, which=which)
        kept = {0: ([], []), 1: ([], [])}
        sizes, per_object = [], []
        for mesh, gt_normals, prepared in objects:
            ctx.upload_ground_truth(mesh, gt_normals)
            first = [trainer.count(w)[0] for w in (0, 1)]
            here = {0: ([], []), 1: ([], [])}
            counts = [0, 0]
            for xyz, normals, cam, rounds, which in prepared:
                ctx.upload_cloud(xyz, normals, cam, np.zeros((1, 3)))
                t0 = time.perf_counter()
                if route == "A":
                    got = ctx.label_view(rounds, gd.MIN_GRASPS, gd.MAX_GRASPS)
                    here[which][0].append(got["images"])
                    here[which][1].append(got["labels"])
                else:
                    got = trainer.append_view(ctx, rounds, gd.MIN_GRASPS, gd.MAX_GRASPS, which=which)
                ms += (time.perf_counter() - t0) * 1e3
                counts[which] += got["num_out"]
                d2h += got["d2h_bytes"]
                h2d += rounds.nbytes
                outs.append(got)
            sizes += counts
            per_object.append((first, counts, here))
        orders = api.shuffle_orders(gd.SHUFFLE_SEED, sizes)  # one stream: per object the training set's order, then the test set's
        t0 = time.perf_counter()
        for i, (first, counts, here) in enumerate(per_object):
            for w in (0, 1):
                order = orders[2 * i + w]
                if route == "A":
                    kept[w][0].append(np.concatenate(here[w][0])[order])
                    kept[w][1].append(np.concatenate(here[w][1])[order])
                else:
                    trainer.reorder(first[w], order, which=w)
                    h2d += order.nbytes
        if route == "A":
            for w in (0, 1):
                img, lab = np.concatenate(kept[w][0]), np.concatenate(kept[w][1])
                trainer.set_data(img, lab, which=w)
                h2d += img.nbytes + lab.nbytes
        ms += (time.perf_counter() - t0) * 1e3
        return ms, d2h, h2d, outs

    def sets():
        return [trainer.get_data(which=w) for w in (0, 1)]

    a = one_pass("A")
    sets_a = sets()
    b = one_pass("B")
    sets_b = sets()
    same = all(x.tobytes() == y.tobytes() for sa, sb in zip(sets_a, sets_b) for x, y in zip(sa, sb))
    assert same and len(sets_a[0][1]) > 0 and len(sets_a[1][1]) > 0, "the two routes disagree"
    times = {"A": [], "B": []}
    for i in range(WARMUP + REPEATS):
        for route in ("A", "B"):
            ms = one_pass(route)[0]
            if i >= WARMUP:
                times[route].append(ms / num_views)
    image_bytes = sum(len(s[1]) for s in sets_a) * 3600 * C
    res = dict(objects=len(objects), views=num_views, channels=C, samples_per_round=gd.NUM_SAMPLES, max_grasps_per_view=gd.MAX_GRASPS,
               n_train=len(sets_a[0][1]), n_test=len(sets_a[1][1]), image_bytes_of_both_sets=image_bytes, warmup=WARMUP, repeats=REPEATS,
               same_bytes=bool(same))
    for route in times:
        t = np.array(times[route])
        res["route_%s_ms_per_view" % route] = dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()))
    res["pcie_bytes"] = dict(A=dict(d2h=int(a[1]), h2d=int(a[2])), B=dict(d2h=int(b[1]), h2d=int(b[2])))
    res["speedup_median"] = res["route_A_ms_per_view"]["median"] / res["route_B_ms_per_view"]["median"]
    trainer.close()
    ctx.close()
    line = json.dumps(res, indent=1)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
