"""Timing of Cloud::sampleAbovePlane on the device (gpd_hip_sample_above_plane) against the host model
(hostlib.sample_above_plane, one core) on voxelised table_mug, raw table_mug and the config-4 300k cloud.  Prints one
JSON line: per cloud the points, the inliers, the median wall time of the device call (it synchronises: launches, the
copies between them and the host's stop rule / refinement included) and of the host model.  Kernel times come from a
separate `rocprofv3 --kernel-trace --stats` run of this script.  GPD_HIP_LIB=libgpd_hip_prof.so with
GPD_PLANE_REFINE=device measures the refinement's sums on one wave instead of the host.

    python profiles/plane_fit_bench.py [--reps 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpd_amd import api, hostlib, synth  # noqa: E402


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    ctx = api.Context(api.default_params(15))
    raw = np.load(os.path.join(ROOT, "tests", "golden", "table_mug_xyz.npz"))["xyz"]
    vox = ctx.preprocess_cloud(raw, voxel_size=0.003)[0]
    big = synth.make_cloud(1234, 300000, clutter=True)["xyz"]
    out = {"refine": os.environ.get("GPD_PLANE_REFINE", "host"), "lib": os.path.basename(api.LIB_PATH)}
    for name, xyz in (("table_mug_voxelised", vox), ("table_mug_raw", raw), ("config4_300k", big)):
        ctx.upload_cloud(xyz, np.zeros_like(xyz))
        dev = ctx.sample_above_plane()
        host = hostlib.sample_above_plane(xyz)
        equal = bool(np.array_equal(dev[0], host[0]) and dev[1].tobytes() == host[1].tobytes() and dev[2:] == host[2:])
        out[name] = dict(points=len(xyz), inliers=dev[2], iterations=dev[3], equal=equal,
                         device_call_ms=round(_median_ms(ctx.sample_above_plane, a.reps), 4),
                         host_model_ms=round(_median_ms(lambda: hostlib.sample_above_plane(xyz), a.host_reps), 4))
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
