#!/usr/bin/env python
"""A resident training step at batch 64 under one recipe, measured the way profiles/train_step_ab.py measures its device route:
Trainer.steps with 50 steps enqueued back to back and one wait, host clock around the call, 3 warm-ups, then 24 repeats; median
and min - max of the time per step, for C = 15 and C = 3.

  python profiles/train_caffe_step.py {net-adam|caffe-sgd} LABEL OUT.json [PACKAGE_ROOT]

net-adam is the trainer without a recipe (Net, Adam), so it runs on a checkout from before the recipes existed too:
PACKAGE_ROOT names the tree whose gpd_amd package and library are measured (default: this one).  One process measures one
(recipe, tree) pair and appends its result to OUT.json; an A/B of two builds is this script run on both trees in turn, in one
session on one machine.  Comparisons are between those runs only, never against figures from another day.
"""
import json
import os
import sys
import time

import numpy as np

REPEATS, WARMUP, STEPS, BATCH, N = 24, 3, 50, 64, 3200


def measure(api, recipe_name, C):
    rng = np.random.RandomState(C)
    img = rng.randint(0, 256, (N, 60, 60, C)).astype(np.uint8)
    img[rng.rand(N, 60, 60, C) < 0.6] = 0
    lab = rng.randint(0, 2, N).astype(np.uint8)
    idx = np.arange(STEPS * BATCH, dtype=np.int32).reshape(STEPS, BATCH)
    ctx = api.Context(api.default_params(C))
    if recipe_name == "caffe-sgd":
        tr = api.Trainer(ctx, recipe=api.train_default_recipe(1), max_batch=BATCH, lr=api.CAFFE_BASE_LR)
        st = api.init_xavier(C, 1)
    else:
        tr = api.Trainer(ctx, max_batch=BATCH)
        st = api.init_state(C, 1)
    tr.set_data(img, lab)
    times, first = [], None
    for i in range(WARMUP + REPEATS):
        tr.set_state(st)  # every repeat walks the same 50 steps from the same state
        t0 = time.perf_counter()
        losses = tr.steps(idx)
        dt = (time.perf_counter() - t0) * 1e3 / STEPS
        first = float(losses[0]) if first is None else first
        assert np.isfinite(losses).all()
        if i >= WARMUP:
            times.append(dt)
    kernels = dict(tr.step_timed(idx[0]))
    tr.close()
    ctx.close()
    t = np.array(times)
    return dict(channels=C, batch=BATCH, steps_per_repeat=STEPS, repeats=REPEATS, first_loss=first, last_loss=float(losses[-1]),
                ms_per_step=dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max())), kernel_ms_one_step=kernels)


def main():
    recipe_name, label, out = sys.argv[1], sys.argv[2], sys.argv[3]
    root = os.path.abspath(sys.argv[4]) if len(sys.argv) > 4 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if recipe_name not in ("net-adam", "caffe-sgd"):
        sys.exit(__doc__)
    sys.path.insert(0, root)
    from gpd_amd import api
    import torch  # only for the device's name
    res = dict(label=label, recipe=recipe_name, device_name=torch.cuda.get_device_name(0), runs=[measure(api, recipe_name, 15), measure(api, recipe_name, 3)])
    done = []
    if os.path.exists(out):
        with open(out) as f:
            done = json.load(f)
    done.append(res)
    with open(out, "w") as f:
        f.write(json.dumps(done, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
