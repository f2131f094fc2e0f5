#!/usr/bin/env python
"""The two arithmetics of the shape-general LeNet route side by side: GPD_LENET_NET_CHAIN (f32 chains on
v_mfma_f32_32x32x2_f32) and GPD_LENET_NET_SPLIT (v_mfma_f32_16x16x32_bf16 on exactly split operands), on bench.py's config-2
candidate list (5000 images, 15 channels).  ONE process, legs alternating over three rounds; per leg 3 warm-up and 20 timed
gpd_hip_replay(2), each read back on its own (ms per pass), HIP events around the scoring pass and behind conv1 / conv2 / fc1
(`rest` = fc2 + logits).

  general chain / general split   A' = [6, 16, 120, 84] (NetCCFFF), C = [40, 100, 500], D = [20, 50, 500] (the stock shape)
  stock kernels                   D in GPD_LENET_F32_CHAIN and GPD_LENET_SPLIT (tuned for 20 / 50 / 500)

Before anything is timed the scores of every leg are asserted as the tests assert them: chain legs bit for bit the fmaf-chain
network (tests/lenet_net_ref.py), the split leg within 4 chain errors + 2 spacings of the float64 network, the stock split
within 1e-4.  At the end: the split leg's median pass must lie below the chain leg's minimum at each shape.

    python profiles/lenet_net_split_ab.py          (needs the GPU; writes profiles/lenet_net_split_ab.json)
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
PEAK_BF16 = 2.5e15  # dense bf16 flop/s of the chip

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
img, cand = ctx.images(hands)  # downloaded once for the checks; the replays use the device copy
n = len(cand)
print("candidates", n, flush=True)

chains = {k: R.chain_batch(oracle, SHAPES[k], R.numpy_route_arrays(states[k]), img[:N_CHECK])["score"] for k in SHAPES}
truths = {k: R.forward(states[k], img[:N_CHECK], torch.float64)["score"] for k in SHAPES}


def executed_products(shape):
    """Piece products the split kernels execute per image, padding included: 16-filter / 16-unit tiles, 8-channel chunks of
    28 taps, fc1's k = 144 round_up(F2, 8), fc2's k in steps of 32; conv1 three products per term, the others six"""
    Cn, F1, F2, H1, H2 = shape
    up = lambda v, m: (v + m - 1) // m * m
    conv1 = up(F1, 16) * 3136 * up(Cn, 8) * 28 * 3
    conv2 = up(F2, 16) * 576 * up(F1, 8) * 28 * 6
    fc1 = up(H1, 16) * 144 * up(F2, 8) * 6
    fc2 = up(H2, 16) * up(H1, 32) * 6 if H2 else 0
    return conv1 + conv2 + fc1 + fc2


def check_chain(sc, k):
    assert np.array_equal(sc[:N_CHECK], chains[k]), k


def check_split(sc, k):
    e_chain, e_split = float(np.abs(chains[k] - truths[k]).max()), float(np.abs(sc[:N_CHECK] - truths[k]).max())
    allow = 4.0 * e_chain + 2.0 * float(np.spacing(np.float32(np.abs(truths[k]).max())))
    assert e_split <= allow, (k, e_split, e_chain, allow)


def leg_general(mode):
    def f(k):
        ctx.set_lenet_net(states[k], net_mode=mode)
        return check_chain if mode == api.LENET_NET_CHAIN else check_split
    return f


def leg_stock(mode):
    def f(k):
        ctx.set_lenet_torch(states[k])
        ctx.set_lenet_mode(mode)
        if mode == api.LENET_F32_CHAIN:
            return check_chain
        return lambda sc, k: np.testing.assert_allclose(sc[:N_CHECK], chains[k], rtol=0, atol=1e-4)
    return f


LEGS = [(route, k, leg_general(mode)) for k in ("A'", "C", "D")
        for route, mode in (("general chain", api.LENET_NET_CHAIN), ("general split", api.LENET_NET_SPLIT))]
LEGS += [("stock f32 chain", "D", leg_stock(api.LENET_F32_CHAIN)), ("stock split", "D", leg_stock(api.LENET_SPLIT))]
rows = []
for rnd in range(ROUNDS):
    for route, k, setup in LEGS:
        check = setup(k)
        ctx.replay(2)
        _, _, _, sc = ctx.replay_times(n_scores=n)
        check(sc, k)
        for _ in range(WARM):
            ctx.replay(2)
        ctx.replay_times()
        passes, kms = [], []
        for _ in range(REPS):
            ctx.replay(2)
            _, net_ms, launches, _ = ctx.replay_times()
            passes.append(net_ms / launches)
            kms.append([x / launches for x in ctx.replay_kernel_ms()])
        km = np.median(np.array(kms), axis=0)
        row = dict(round=rnd, route=route, shape=k, widths=list(SHAPES[k][1:]), images=n, pass_ms=passes, conv1_ms=float(km[0]), conv2_ms=float(km[1]),
                   fc1_ms=float(km[2]), rest_ms=float(km[3]))
        rows.append(row)
        print(json.dumps(dict(row, pass_ms=float(np.median(passes)))), flush=True)
ctx.close()

summary = {}
for r in rows:
    s = summary.setdefault("%s %s" % (r["route"], r["shape"]), dict(pass_ms=[], k=[]))
    s["pass_ms"] += r["pass_ms"]
    s["k"].append([r["conv1_ms"], r["conv2_ms"], r["fc1_ms"], r["rest_ms"]])
for key, s in summary.items():
    k = np.median(np.array(s.pop("k")), axis=0)
    p = np.array(s.pop("pass_ms"))
    s.update(median_ms=float(np.median(p)), min_ms=float(p.min()), max_ms=float(p.max()), conv1_ms=float(k[0]), conv2_ms=float(k[1]), fc1_ms=float(k[2]),
             rest_ms=float(k[3]))
for k, shape in SHAPES.items():
    s = summary["general split %s" % k]
    s["executed_piece_products_per_image"] = executed_products(shape)
    s["share_of_bf16_peak"] = 2.0 * executed_products(shape) * n / (s["median_ms"] * 1e-3) / PEAK_BF16
    s["speedup_over_chain_median"] = summary["general chain %s" % k]["median_ms"] / s["median_ms"]
json.dump(dict(protocol="one process, legs alternating, %d rounds of %d warm-up + %d timed gpd_hip_replay(2) per leg, each read back on its own; device "
                        "events; medians and min-max over all %d timed calls of a leg" % (ROUNDS, WARM, REPS, ROUNDS * REPS),
               images=n, channels=C, rows=rows, summary=summary), open(os.path.join(ROOT, "profiles", "lenet_net_split_ab.json"), "w"), indent=1)
print(json.dumps(summary, indent=1), flush=True)
for k in SHAPES:
    split, chain = summary["general split %s" % k], summary["general chain %s" % k]
    assert split["median_ms"] < chain["min_ms"], (k, split["median_ms"], chain["min_ms"])
print("split median < chain minimum at every shape", flush=True)
