#!/usr/bin/env python
"""The shape-general LeNet route (gpd_hip_set_lenet_net) against the stock kernels and PyTorch-ROCm eager, on bench.py's
config-2 candidate list (5000 images, 15 channels), routes alternating in ONE process: per leg 3 warm-up + 20 timed
gpd_hip_replay(2), HIP events around the scoring pass and behind conv1 / conv2 / fc1 (ms per pass; `rest` = fc2 + logits).

  general route   A' = [6, 16, 120, 84] (NetCCFFF), C = [40, 100, 500], D = [20, 50, 500] (the stock shape)
  stock kernels   D in GPD_LENET_F32_CHAIN (the same arithmetic, tiled for 20 / 50 / 500) and GPD_LENET_SPLIT
  torch eager     float32 forward of the same networks on the same images (device events, same warm-up and repeats)

The first 4 scores of every leg are held against the fmaf-chain network (tests/lenet_net_ref.py) before anything is timed:
bit for bit for the general route and the chain mode, within 1e-4 for the split mode.

    python profiles/lenet_net_ab.py          (needs the GPU; writes profiles/lenet_net_ab.json)
"""
import json, os, sys
import numpy as np
import torch  # before libgpd_hip.so: torch brings its own HIP runtime, and the one loaded second finds no device
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench
import oracle
import lenet_net_ref as R
from gpd_amd import api, synth

preset = bench.CONFIGS["2"]
C, points, candidates = preset["channels"], preset["points"], preset["candidates"]
SHAPES = {"A'": (C, 6, 16, 120, 84), "C": (C, 40, 100, 500, 0), "D": (C, 20, 50, 500, 0)}
states = {k: R.make_state(v, 100 + i) for i, (k, v) in enumerate(sorted(SHAPES.items()))}
WARM, REPS, ROUNDS, N_CHECK = 3, 20, 3, 4

torch.zeros(1, device="cuda")
ctx = api.Context(api.default_params(C))
ctx.set_lenet_torch(states["D"])
cloud = synth.make_cloud(1234, points, clutter=preset["clutter"])
ctx.upload_cloud(cloud["xyz"], cloud["normals"], cloud["cam_source"], cloud["view_points"])
si = synth.sample_indices(cloud, min(int(candidates / 2.0) + 64, int(cloud["is_object"].sum())))
hands = ctx.search(si).copy()
bench._filter_workspace(hands, ctx.params)
flat = hands.reshape(-1)
vidx = np.flatnonzero(flat["valid"])
if len(vidx) > candidates:
    flat["valid"][vidx[candidates:]] = 0
img, cand = ctx.images(hands)  # downloaded once (the checks and torch read them); the replays use the device copy
n = len(cand)
print("candidates", n, flush=True)

chains = {k: R.chain_batch(oracle, SHAPES[k], R.numpy_route_arrays(states[k]), img[:N_CHECK])["score"] for k in SHAPES}


def leg_general(k):
    ctx.set_lenet_net(states[k])
    return ctx.lenet_net_info()["macs_per_image"], 0.0


def leg_stock(mode):
    def f(k):
        ctx.set_lenet_torch(states[k])
        ctx.set_lenet_mode(mode)
        return 20 * 3136 * C * 25 + 50 * 576 * 500 + 7200 * 500 + 1000, (0.0 if mode == api.LENET_F32_CHAIN else 1e-4)
    return f


LEGS = [("general", "A'", leg_general), ("general", "C", leg_general), ("general", "D", leg_general),
        ("stock f32 chain", "D", leg_stock(api.LENET_F32_CHAIN)), ("stock split", "D", leg_stock(api.LENET_SPLIT))]
rows = []
for rnd in range(ROUNDS):
    for route, k, setup in LEGS:
        macs, tol = setup(k)
        ctx.replay(2)
        _, _, _, sc = ctx.replay_times(n_scores=n)
        err = float(np.abs(sc[:N_CHECK] - chains[k]).max())
        assert err <= tol, (route, k, err)
        for _ in range(WARM):
            ctx.replay(2)
        ctx.replay_times()
        for _ in range(REPS):
            ctx.replay(2)
        _, net_ms, launches, _ = ctx.replay_times()
        km = [x / launches for x in ctx.replay_kernel_ms()]
        ms = net_ms / launches
        row = dict(round=rnd, route=route, shape=k, widths=list(SHAPES[k][1:]), images=n, ms=ms, conv1_ms=km[0], conv2_ms=km[1], fc1_ms=km[2],
                   rest_ms=km[3], macs_per_image=macs, tmacs_per_s=macs * n / ms * 1e-9)
        rows.append(row)
        print(json.dumps(row), flush=True)
ctx.close()

dev = torch.device("cuda")
x_u8 = torch.from_numpy(np.ascontiguousarray(np.transpose(img, (0, 3, 1, 2)))).to(dev)
for rnd in range(ROUNDS):
    for k in sorted(SHAPES):
        t = {key: torch.from_numpy(v.copy()).to(dev) for key, v in states[k].items()}
        F = torch.nn.functional

        def fwd():
            with torch.no_grad():
                x = x_u8.float() * R.INPUT_SCALE
                p1 = F.relu(F.max_pool2d(F.conv2d(x, t["conv1.weight"], t["conv1.bias"]), 2))
                p2 = F.relu(F.max_pool2d(F.conv2d(p1, t["conv2.weight"], t["conv2.bias"]), 2))
                a = F.relu(F.linear(p2.reshape(len(x), -1), t["fc1.weight"], t["fc1.bias"]))
                if "fc3.weight" in t:
                    a = F.relu(F.linear(a, t["fc2.weight"], t["fc2.bias"]))
                    y = F.linear(a, t["fc3.weight"], t["fc3.bias"])
                else:
                    y = F.linear(a, t["fc2.weight"], t["fc2.bias"])
                return y[:, 1] - y[:, 0]
        sc = fwd().cpu().numpy()
        assert np.abs(sc[:N_CHECK] - chains[k]).max() <= 1e-3
        for _ in range(WARM):
            fwd()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fwd()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / REPS
        row = dict(round=rnd, route="torch eager f32", shape=k, widths=list(SHAPES[k][1:]), images=n, ms=ms)
        rows.append(row)
        print(json.dumps(row), flush=True)

summary = {}
for r in rows:
    summary.setdefault("%s %s" % (r["route"], r["shape"]), []).append(r["ms"])
summary = {k: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v))) for k, v in summary.items()}
json.dump(dict(protocol="one process, routes alternating, %d rounds of %d warm-up + %d timed passes, device events" % (ROUNDS, WARM, REPS),
               images=n, channels=C, rows=rows, summary=summary), open(os.path.join(ROOT, "profiles", "lenet_net_ab.json"), "w"), indent=1)
print(json.dumps(summary), flush=True)
