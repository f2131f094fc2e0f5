#!/usr/bin/env python
"""SequentialImportanceSampling::detectGrasps, two routes, alternating in one process:

  resident  Context.detect_sis: the rounds, the draws' selection, the accumulated hand sets, one LeNet pass, the cut at min_score
            and the clustering on the device; per round only small words come back, the records leave in one copy
  composed  the public calls that existed before it, as the host loop composes them: search, then per round the draw on the host
            (the same seeded streams: api.sis_proposals / api.sis_select), search_samples, the workspace filter on the host;
            then, as pruneGraspCandidates does for a list collected over several searches, search_samples over every collected
            hand set a second time, images with the collected flags, score, the cut, find_clusters

on the 30 000-point scene, C = 15, the cfg defaults of the driver (prob_rand_samples 0.3, sigma 0.02, sum of Gaussians,
min_score 0, min_inliers 1) at two sizes: 50 + 5 x 50 samples (the cfg defaults) and 2000 + 5 x 2000.  Host clock around each
route (both end in a synchronise), median and spread of REPEATS runs after a warm-up.  The two routes must return the same bytes.
   python profiles/sis_ab.py [out.json]
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

REPEATS, WARMUP, CHANNELS, ITERATIONS = 24, 3, 15, 5
PROB, SIGMA, METHOD, MIN_SCORE, MIN_INLIERS, SEED = 0.3, 0.02, 0, 0.0, 1, 7
WS = (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0)
HAND = api.HAND_DTYPE.itemsize


def live_sets(op, hands):
    hands = oracle.filter_workspace(op, hands)
    return hands[hands["valid"].astype(bool).any(axis=1)]


def draw_host(r, centres, init, xyz, per):
    nr = int(PROB * per)
    ng = per - nr
    st, first, block = None, [0, 0], 2 * per + 64
    while st is None or st["shortfall"] > 0:
        g = api.sis_proposals(SEED, r, 0, first[0], block if st is None or st["accepted"][0] < ng else 0, SIGMA)
        u = api.sis_proposals(SEED, r, 1, first[1], block if st is None or st["accepted"][1] < nr else 0)
        first = [first[0] + len(g), first[1] + len(u)]
        st = api.sis_select(centres, g, u, init, xyz, WS, METHOD, ng, nr, st)
    return st["samples"]


def measure(ctx, op, cl, n_init, per):
    init = synth.sample_indices(cl, n_init).astype(np.int32)
    slots = ctx.n_slots

    def resident():
        return ctx.detect_sis(init, ITERATIONS, per, PROB, SIGMA, METHOD, MIN_SCORE, WS, MIN_INLIERS, False, SEED)

    def composed():
        d2h = 0
        sets = [live_sets(op, ctx.search(init))]
        d2h += len(init) * (slots * HAND + 32)
        for r in range(ITERATIONS):
            centres = np.concatenate([s[:, 0]["sample"] for s in sets])
            if not len(centres):
                break
            samples = draw_host(r, centres, init, cl["xyz"], per)
            sets.append(live_sets(op, ctx.search_samples(samples)))
            d2h += per * (slots * HAND + 32)
        allh = np.concatenate(sets)
        fresh = ctx.search_samples(allh[:, 0]["sample"])  # the second search of every collected hand set
        d2h += len(allh) * (slots * HAND + 32)
        fresh["valid"] = allh["valid"]
        fresh["set_index"] = np.arange(len(fresh), dtype=np.int32)[:, None]
        _, cand = ctx.images(fresh, download=False)
        scores = ctx.score(None, n=len(cand))
        d2h += cand.nbytes + scores.nbytes
        recs = fresh.reshape(-1)[cand].copy()
        recs["score"] = scores
        recs = recs[scores > np.float64(MIN_SCORE)]
        if MIN_INLIERS > 0 and len(recs):
            recs, _, _ = ctx.find_clusters(recs, recs["score"].astype(np.float64), MIN_INLIERS, False)
            d2h += len(recs) * (HAND + 12)
        return dict(hands=recs, d2h_bytes=d2h, num_sets=len(allh), num_candidates=len(cand))

    a, b = resident(), composed()
    same = a["hands"].tobytes() == b["hands"].tobytes()
    assert same and a["num_candidates"] == b["num_candidates"] and a["num_sets"] == b["num_sets"], "the two routes disagree"
    times = {"resident": [], "composed": []}
    stage = []
    for i in range(WARMUP + REPEATS):
        for name, fn in (("resident", resident), ("composed", composed)):
            t0 = time.perf_counter()
            out = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= WARMUP:
                times[name].append(dt)
                if name == "resident":
                    stage.append(out["stage_ms"])
    res = dict(num_init_samples=n_init, num_iterations=ITERATIONS, num_samples=per, num_sets=a["num_sets"], num_candidates=a["num_candidates"],
               num_hands=a["num_hands"], round_counts=a["round_counts"].tolist(), same_bytes=bool(same))
    for name in times:
        t = np.array(times[name])
        res[name + "_ms"] = dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()), p25=float(np.percentile(t, 25)),
                                 p75=float(np.percentile(t, 75)))
    res["resident_stage_ms_median"] = dict(zip(("draw", "search", "images_accumulate", "lenet_select_cluster"),
                                               np.median(np.array(stage), axis=0).tolist()))
    res["d2h_bytes"] = dict(resident=int(a["d2h_bytes"]), composed=int(b["d2h_bytes"]))
    res["speedup_median"] = res["composed_ms"]["median"] / res["resident_ms"]["median"]
    return res


def main():
    cl = synth.make_cloud(1234, 30000)
    real = dict(np.load(os.path.join(ROOT, "tests", "golden", "lenet15_params.npz")))
    weights = synth.lenet_weights(CHANNELS, real=real, trained_magnitude=True)
    op = oracle.default_params(CHANNELS)
    ctx = api.Context(api.default_params(CHANNELS))
    ctx.set_lenet_weights(weights)
    ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
    res = dict(points=30000, channels=CHANNELS, repeats=REPEATS, warmup=WARMUP, prob_rand_samples=PROB, sigma=SIGMA, sampling_method=METHOD,
               min_score=MIN_SCORE, min_inliers=MIN_INLIERS, seed=SEED,
               sizes=[measure(ctx, op, cl, 50, 50), measure(ctx, op, cl, 2000, 2000)])
    ctx.close()
    line = json.dumps(res, indent=1)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
