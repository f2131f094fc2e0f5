"""python profiles/train_net_step.py OUT.json — gpd_hip_train_step_timed at batch 64, C = 15, for three networks of the
family: five repeats of ten timed steps each; per repeat the median over its steps of the sum of the kernels'
event times and of each kernel's.  The spread over the five repeats is what a comparison between commits has to exceed."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpd_amd import api  # noqa: E402

SHAPES = [(20, 50, 500, 0), (40, 100, 500, 0), (6, 16, 120, 84)]
C, B, REPEATS, STEPS = 15, 64, 5, 10


def main(out_path):
    rng = np.random.RandomState(11)
    img = rng.randint(0, 256, (70, 60, 60, C)).astype(np.uint8)
    img[rng.rand(*img.shape) < 0.6] = 0
    lab = np.random.RandomState(12).randint(0, 2, 70).astype(np.uint8)
    idx = (np.arange(B) % 70).astype(np.int32)
    runs = []
    for widths in SHAPES:
        ctx = api.Context(api.default_params(C), device=0)
        # the first shape through the stock entry, as every earlier commit creates it
        t = api.Trainer(ctx, api.train_default_params(C, B), shape=None if widths == SHAPES[0] else widths)
        t.set_data(img, lab)
        t.set_state(api.init_state(C, 1, shape=widths))
        for _ in range(3):
            t.step_timed(idx)
        totals, kernels = [], []
        for _ in range(REPEATS):
            steps = [t.step_timed(idx) for _ in range(STEPS)]
            totals.append(float(np.median([sum(ms for _, ms in s) for s in steps])))
            kernels.append({name: float(np.median([s[i][1] for s in steps])) for i, (name, _) in enumerate(steps[0])})
        runs.append(dict(shape=[C] + list(widths), batch=B, launches=len(kernels[0]), parameters=int(sum(api.net_sizes(t.shape))),
                         step_ms_per_repeat=totals, step_ms_median=float(np.median(totals)), step_ms_spread=max(totals) - min(totals),
                         kernel_ms_median={k: float(np.median([r[k] for r in kernels])) for k in kernels[0]}))
        t.close()
        ctx.close()
    with open(out_path, "w") as f:
        json.dump(dict(what="step_timed: sum of the kernels' event times, ms", repeats=REPEATS, steps_per_repeat=STEPS, runs=runs), f, indent=1)
    for r in runs:
        print(r["shape"], r["step_ms_per_repeat"])


if __name__ == "__main__":
    main(sys.argv[1])
