#!/usr/bin/env python
"""Scores of hand sets the caller holds, two routes, alternating in one process:

  given     Context.score_given: neighbourhood lists around the sets' samples, the caller's records to the device, images, LeNet;
            one score and one index per candidate come back
  composed  the public calls that existed before it, as GraspDetector::pruneGraspCandidates composed them for a list that is not
            the last search's: search_samples over the sets' samples (a complete second hand search, its records downloaded),
            images with the caller's flags, score

on the benchmark's workload (bench.py, configuration 2): the 30 000-point scene, 2564 hand sets, the first 5000 valid candidates
after the workspace filter, C = 15.  Host clock around each route (both end in a synchronise), median and spread of REPEATS runs
after a warm-up; bytes across PCIe counted from the calls' arguments.  The two routes must return the same scores.
   python profiles/given_ab.py [out.json]
   python profiles/given_ab.py --once      one score_given call and nothing timed (for a kernel trace)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402  (the host workspace filter)
from gpd_amd import api, synth  # noqa: E402

REPEATS, WARMUP, CHANNELS, POINTS, CANDIDATES = 24, 3, 15, 30000, 5000
HAND = api.HAND_DTYPE.itemsize


def main():
    once = "--once" in sys.argv[1:]
    out_path = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    cl = synth.make_cloud(1234, POINTS)
    real = dict(np.load(os.path.join(ROOT, "tests", "golden", "lenet15_params.npz")))
    weights = synth.lenet_weights(CHANNELS, real=real, trained_magnitude=True)
    ctx = api.Context(api.default_params(CHANNELS))
    ctx.set_lenet_weights(weights)
    ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
    si = synth.sample_indices(cl, min(CANDIDATES // 2 + 64, int(cl["is_object"].sum())))
    op = oracle.default_params(CHANNELS)
    # --once: the hand sets come from the CPU oracle, so that the trace of the process holds no hand search at all
    found = oracle.search(op, cl["xyz"], cl["normals"], si) if once else ctx.search(si)
    hands = oracle.filter_workspace(op, found)
    flat = hands.reshape(-1)
    vidx = np.flatnonzero(flat["valid"])
    flat["valid"][vidx[CANDIDATES:]] = 0
    S, slots = hands.shape
    samples = np.ascontiguousarray(hands[:, 0]["sample"])

    def given():
        out, scores, cand, _ = ctx.score_given(hands)
        return scores, cand, out.reshape(-1)[cand]

    def composed():
        fresh = ctx.search_samples(samples)
        assert len(fresh) == S
        fresh["valid"] = hands["valid"]
        _, cand = ctx.images(fresh, download=False)
        scores = ctx.score(None, n=len(cand))
        recs = fresh.reshape(-1)[cand]
        recs["score"] = scores
        return scores, cand, recs

    if once:
        scores, cand, _ = given()
        print("score_given: %d sets, %d candidates" % (S, len(cand)))
        ctx.close()
        return
    a, b = given(), composed()
    n = len(a[1])
    same = a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
    assert same and n == CANDIDATES, "the two routes disagree"
    # the records differ in nothing the image stage reads; set_index is the composed route's own numbering
    for f in ("sample", "frame", "bottom", "center", "score"):
        assert a[2][f].tobytes() == b[2][f].tobytes(), f
    times = {"given": [], "composed": []}
    stage = {"given": [], "composed": []}
    for i in range(WARMUP + REPEATS):
        for name, fn in (("given", given), ("composed", composed)):
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= WARMUP:
                times[name].append(dt)
                stage[name].append([float(x) for x in ctx.stage_ms()])
    res = dict(points=POINTS, channels=CHANNELS, num_sets=int(S), slots=int(slots), num_candidates=int(n), repeats=REPEATS, warmup=WARMUP,
               same_scores=bool(same))
    for name in times:
        t = np.array(times[name])
        res[name + "_ms"] = dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()), p25=float(np.percentile(t, 25)),
                                 p75=float(np.percentile(t, 75)))
    # HIP events of the calls: given [1] = lists + ingest + plan + images, [2] = LeNet; composed [0] = the search, [1] = plan + images, [2] = LeNet
    res["given_stage_ms_median"] = dict(zip(("lists_images", "lenet"), np.median(np.array(stage["given"]), axis=0)[1:].tolist()))
    res["composed_stage_ms_median"] = dict(zip(("search", "images", "lenet"), np.median(np.array(stage["composed"]), axis=0).tolist()))
    res["pcie_bytes"] = dict(
        given=dict(h2d=int(S * 24 + S * slots * HAND), d2h=int(S * 32 + 8 * n)),
        composed=dict(h2d=int(S * 24 + S * slots + S * 24), d2h=int(S * (slots * HAND + 32) + 8 * n)))
    res["speedup_median"] = res["composed_ms"]["median"] / res["given_ms"]["median"]
    ctx.close()
    line = json.dumps(res, indent=1)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
