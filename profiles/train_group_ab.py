#!/usr/bin/env python
"""A training step over G = 2 replicas at a global batch of 64 (32 images each), three routes, alternating passes in one process:

  A  the composed route, the definition: Trainer.gradients on each replica (a parameter-sized buffer to the host), the
     fixed-order mean on the host (api.train_group_mean per tensor), Trainer.apply on each replica (the buffer back)
  B  TrainerGroup.steps: the same mean formed on the devices, a slice per replica (gpd_hip_train_group_steps)
  C  for scale only: ONE trainer at batch 64 (Trainer.steps), the single-device route

at C = 15 and C = 3, both replicas on device 0 (each on a context of its own) and, where the machine shows two devices, on
devices 0 and 1.  A pass is STEPS steps; its time over STEPS is the per-step figure.  Host clock around calls that end in a
synchronise.  WARMUP passes of each route, then REPEATS; median and min - max.  Before any timing A and B run from one state
and must leave the same bytes in both replicas.   python profiles/train_group_ab.py [out.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gpd_amd import api  # noqa: E402

REPEATS, WARMUP, STEPS = 20, 3, 4
G, BATCH, N_IMAGES = 2, 64, 256


def everything(t):
    s = t.get_solver_state()
    return [v.tobytes() for v in t.get_state().values()] + [v.tobytes() for v in s["m"].values()] + [v.tobytes() for v in s["v"].values()] + [s["count"]]


def measure(C, devices):
    rng = np.random.RandomState(C)
    img = rng.randint(0, 256, (N_IMAGES, 60, 60, C)).astype(np.uint8)
    img[rng.rand(*img.shape) < 0.6] = 0
    lab = rng.randint(0, 2, N_IMAGES).astype(np.uint8)
    b = BATCH // G
    ctxs = [api.Context(api.default_params(C), device=d) for d in devices] + [api.Context(api.default_params(C), device=devices[0])]
    trainers = [api.Trainer(c, max_batch=b) for c in ctxs[:G]]
    single = api.Trainer(ctxs[G], max_batch=BATCH)
    group = api.TrainerGroup(trainers)
    for r, t in enumerate(trainers):
        t.set_data(img[r::G], lab[r::G])
    single.set_data(img, lab)
    n_params = 500 * C + 3626572
    idx = rng.randint(0, N_IMAGES // G, (G, STEPS, b)).astype(np.int32)
    idx1 = rng.randint(0, N_IMAGES, (STEPS, BATCH)).astype(np.int32)
    moved = {}

    def start():
        trainers[0].set_state(api.init_state(C, 1))
        group.broadcast(0)
        single.set_state(api.init_state(C, 1))

    def route_a():
        for s in range(STEPS):
            got = [t.gradients(idx[r, s]) for r, t in enumerate(trainers)]
            mean = {k: api.train_group_mean([g[k] for g, _ in got]) for k in api.TORCH_KEYS}
            for t in trainers:
                t.apply(mean)
        moved["A"] = dict(between_replicas=0, host_device=STEPS * G * (2 * 4 * n_params + 4 * b + 4))

    def route_b():
        group.steps(idx)
        between, host = group.last_bytes()
        moved["B"] = dict(between_replicas=between, host_device=host)

    def route_c():
        single.steps(idx1)
        moved["C"] = dict(between_replicas=0, host_device=STEPS * (4 * BATCH + 4))

    routes = dict(A=route_a, B=route_b, C=route_c)
    start()
    route_a()
    after_a = [everything(t) for t in trainers]
    start()
    route_b()
    after_b = [everything(t) for t in trainers]
    same = after_a == after_b and after_a[0] == after_a[1] and group.verify() == 0
    assert same, "the composed route and the group disagree"
    times = {k: [] for k in routes}
    for i in range(WARMUP + REPEATS):
        for name, fn in routes.items():
            start()
            t0 = time.perf_counter()
            fn()
            ms = (time.perf_counter() - t0) * 1e3
            if i >= WARMUP:
                times[name].append(ms / STEPS)
    res = dict(channels=C, devices=list(devices), floats_per_buffer=n_params, same_bytes=bool(same))
    for name in routes:
        t = np.array(times[name])
        res["route_%s_ms_per_step" % name] = dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()))
        res["route_%s_bytes_per_step" % name] = {k: v // STEPS for k, v in moved[name].items()}
    res["A_over_B_median"] = res["route_A_ms_per_step"]["median"] / res["route_B_ms_per_step"]["median"]
    res["B_over_C_median"] = res["route_B_ms_per_step"]["median"] / res["route_C_ms_per_step"]["median"]
    group.close()
    for t in trainers + [single]:
        t.close()
    for c in ctxs:
        c.close()
    return res


def main():
    import torch
    two = torch.cuda.device_count() >= 2
    res = dict(replicas=G, global_batch=BATCH, steps_per_pass=STEPS, warmup=WARMUP, repeats=REPEATS, one_device=[], two_devices=[] if two else "not measured")
    for C in (15, 3):
        res["one_device"].append(measure(C, [0, 0]))
        if two:
            res["two_devices"].append(measure(C, [0, 1]))
    line = json.dumps(res, indent=1)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
