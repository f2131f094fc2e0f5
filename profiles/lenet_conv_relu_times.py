#!/usr/bin/env python
"""LeNet stage and its four kernels on bench.py's default candidate list (config 2) with gpd_hip_set_lenet_conv_relu off and on,
three times alternating in one process: 3 warm-up + 20 timed gpd_hip_replay(3) per leg, HIP-event times per step (ms).

    python profiles/lenet_conv_relu_times.py          (needs the GPU; one JSON line per leg)
"""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from gpd_amd import api, synth
preset = bench.CONFIGS["2"]
C, points, candidates = preset["channels"], preset["points"], preset["candidates"]
real = dict(np.load(os.path.join(ROOT, "tests", "golden", "lenet%d_params.npz" % C)))
w = synth.lenet_weights(C, real=real, trained_magnitude=True)
ctx = api.Context(api.default_params(C))
ctx.set_lenet_weights(w)
cloud = synth.make_cloud(1234, points, clutter=preset["clutter"])
ctx.upload_cloud(cloud["xyz"], cloud["normals"], cloud["cam_source"], cloud["view_points"])
n_samples = min(int(candidates / 2.0) + 64, int(cloud["is_object"].sum()))
si = synth.sample_indices(cloud, n_samples)
hands = ctx.search(si)
hands_f = hands.copy()
bench._filter_workspace(hands_f, ctx.params)
flat = hands_f.reshape(-1)
vidx = np.flatnonzero(flat["valid"])
if len(vidx) > candidates:
    flat["valid"][vidx[candidates:]] = 0
_, cand = ctx.images(hands_f, download=False)
print("candidates", len(cand), flush=True)
out = []
for rep in range(3):
    for on in (0, 1):
        ctx.set_lenet_conv_relu(on)
        for _ in range(3):
            ctx.replay(3)
        ctx.replay_times()
        for _ in range(20):
            ctx.replay(3)
        img_ms, net_ms, launches, sc = ctx.replay_times(n_scores=len(cand))
        k = ctx.replay_kernel_ms()
        row = dict(rep=rep, conv_relu=on, lenet_ms=net_ms / launches, image_ms=img_ms / launches, conv1=k[0] / launches, conv2=k[1] / launches,
                   ip1=k[2] / launches, ip2=k[3] / launches, score_mean=float(sc.mean()))
        out.append(row)
        print(json.dumps(row), flush=True)
ctx.close()
