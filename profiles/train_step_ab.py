#!/usr/bin/env python
"""A training step of pytorch/network.py::Net at batch 64, two routes, alternating in one process:

  device  Trainer.steps: 50 resident steps enqueued back to back, one wait (gpd_hip_train_steps)
  torch   PyTorch-ROCm eager: the same Net, nn.CrossEntropyLoss and torch.optim.Adam (lr 1e-3, weight decay 5e-4), float
          batches already on the device, 50 steps, then torch.cuda.synchronize()

for C = 15 and C = 3.  Host clock around each route (both end in a synchronise), 3 warm-ups, then 24 repeats of 50 steps per
route: median and min - max of the time per step.  Both routes start from the same state (init_state) and see the same
batches; their first losses are printed side by side.  Also the device route's per-kernel HIP-event times (one timed step per
repeat, median).  The comparison is against torch, never against an earlier build.   python profiles/train_step_ab.py [out.json]
"""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gpd_amd import api  # noqa: E402

REPEATS, WARMUP, STEPS, BATCH, N = 24, 3, 50, 64, 3200


class Net(nn.Module):  # pytorch/network.py::Net
    def __init__(self, channels):
        super().__init__()
        self.conv1 = nn.Conv2d(channels, 20, 5)
        self.pool = nn.MaxPool2d(2, 2)
        self.conv2 = nn.Conv2d(20, 50, 5)
        self.fc1 = nn.Linear(50 * 12 * 12, 500)
        self.fc2 = nn.Linear(500, 2)

    def forward(self, x):
        x = self.pool(F.relu(self.conv1(x)))
        x = self.pool(F.relu(self.conv2(x)))
        x = x.view(-1, 50 * 12 * 12)
        return self.fc2(F.relu(self.fc1(x)))


def measure(C):
    rng = np.random.RandomState(C)
    img = rng.randint(0, 256, (N, 60, 60, C)).astype(np.uint8)
    img[rng.rand(N, 60, 60, C) < 0.6] = 0
    lab = rng.randint(0, 2, N).astype(np.uint8)
    idx = np.arange(STEPS * BATCH, dtype=np.int32).reshape(STEPS, BATCH)
    st = api.init_state(C, 1)

    ctx = api.Context(api.default_params(C))
    tr = api.Trainer(ctx, max_batch=BATCH)
    tr.set_state(st)
    tr.set_data(img, lab)

    dev = torch.device("cuda:0")
    net = Net(C).to(dev)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()})
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, weight_decay=5e-4)
    crit = nn.CrossEntropyLoss()
    xs = [(torch.from_numpy(np.ascontiguousarray(np.transpose(img[i], (0, 3, 1, 2)))).float() / 256).to(dev) for i in idx]
    ys = [torch.from_numpy(lab[i].astype(np.int64)).to(dev) for i in idx]
    torch.cuda.synchronize()

    def device_route():
        return float(tr.steps(idx)[0])

    def torch_route():
        first = None
        for x, y in zip(xs, ys):
            opt.zero_grad()
            loss = crit(net(x), y)
            loss.backward()
            opt.step()
            first = loss if first is None else first
        torch.cuda.synchronize()
        return float(first.item())

    times = {"device": [], "torch": []}
    first = {}
    kernels = []
    for i in range(WARMUP + REPEATS):
        for name, fn in (("device", device_route), ("torch", torch_route)):
            t0 = time.perf_counter()
            out = fn()
            dt = (time.perf_counter() - t0) * 1e3 / STEPS
            first.setdefault(name, out)
            if i >= WARMUP:
                times[name].append(dt)
        if i >= WARMUP:
            kernels.append(tr.step_timed(idx[0]))
    res = dict(channels=C, batch=BATCH, steps_per_repeat=STEPS, repeats=REPEATS, first_loss=first)
    for name, t in times.items():
        t = np.array(t)
        res[name + "_ms_per_step"] = dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()))
    res["device_over_torch_median"] = res["device_ms_per_step"]["median"] / res["torch_ms_per_step"]["median"]
    names = [k for k, _ in kernels[0]]
    med = np.median(np.array([[ms for _, ms in k] for k in kernels]), axis=0)
    res["device_kernel_ms_median"] = {k: float(v) for k, v in zip(names, med)}
    res["device_kernel_ms_sum"] = float(med.sum())
    tr.close()
    ctx.close()
    return res


def main():
    res = dict(device_name=torch.cuda.get_device_name(0), runs=[measure(15), measure(3)])
    line = json.dumps(res, indent=1)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
