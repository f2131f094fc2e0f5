"""Cloud::removeStatisticalOutliers inside a RAW job of gpd_hip_detect_batch (gpd_detect_job.outlier_mean_k /
outlier_stddev_mult): after the voxeliser, before the normals.

The reference of every comparison is the stepwise route through the single-call entries — gpd_hip_preprocess_cloud, upload,
gpd_hip_remove_statistical_outliers, gpd_hip_estimate_normals, then the search at the same samples — whose outlier step is
proven against the host model in test_gpu_outliers.py.  The raw job is never its own reference."""
import os

import numpy as np
import pytest

from gpd_amd import api, synth
from pyref_sample import dense_fisher_yates

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
WS = np.array([-0.4, 0.4, -0.4, 0.4, -1.0, 1.0])
CELL, RADIUS = 0.003, 0.03


def scan_with_flying_pixels(seed, n):
    """synth.raw_scan plus forty isolated points hovering 6 cm and more over the scene, inside the workspace"""
    scan, sm = synth.raw_scan(seed, n)
    rng = np.random.RandomState(seed + 1)
    top = scan["xyz"][:, 2].max()
    fly = np.stack([rng.uniform(-0.15, 0.15, 40), rng.uniform(-0.15, 0.15, 40), top + rng.uniform(0.06, 0.12, 40)], 1).astype(np.float32)
    at = rng.randint(0, n, 40)
    xyz = np.insert(scan["xyz"], at, fly, axis=0)
    cam = np.insert(scan["cam_source"], at, 1, axis=1)
    return dict(xyz=np.ascontiguousarray(xyz), cam_source=np.ascontiguousarray(cam), view_points=scan["view_points"]), sm


def inside(p, ws):
    return (p[:, 0] > ws[0]) & (p[:, 0] < ws[1]) & (p[:, 1] > ws[2]) & (p[:, 1] < ws[3]) & (p[:, 2] > ws[4]) & (p[:, 2] < ws[5])


def stepwise(ctx, scan, sm, mean_k, mult, draws=0, seed=0):
    vox, cam, _, _ = ctx.preprocess_cloud(scan["xyz"], scan["cam_source"], WS, CELL)
    ctx.upload_cloud(vox, np.zeros_like(vox), cam, scan["view_points"])
    out = dict(voxelised=len(vox), M=len(vox))
    if mean_k > 0:
        kept, _, _ = ctx.remove_statistical_outliers(mean_k, mult)
        out["M"] = len(kept)
    ctx.estimate_normals(RADIUS)
    if sm is not None:
        sm = sm[inside(sm, WS)]
        hands, out["n_cand"] = ctx.detect_samples(sm)
        flat = hands.reshape(-1)
        out["records"], out["S"], out["si"] = flat[flat["valid"].astype(bool)].copy(), len(sm), None
    else:
        si = dense_fisher_yates(out["M"], draws, seed)
        hands, _, out["n_cand"] = ctx.detect_select(si, 0)
        out["records"], out["S"], out["si"] = hands.copy(), len(si), si.astype(np.int32)
    return out


def build(ctx, specs):
    jobs = (api.DetectJob * len(specs))()
    keeps = []
    for i, (scan, sm, mean_k, mult, draws, seed) in enumerate(specs):
        one, keep = ctx.raw_batch([scan], [sm], WS, CELL, RADIUS, num_draws=draws, sample_seed=seed, outlier_mean_k=mean_k,
                                  outlier_stddev_mult=mult)
        jobs[i] = one[0]
        keeps.append(keep[0])
    return jobs, keeps


def run(ctx, jobs, expect_rc=0):
    rc = api.lib().gpd_hip_detect_batch(ctx._h, jobs, len(jobs))
    assert rc == expect_rc, (rc, api.lib().gpd_hip_last_error().decode())


def check(j, keep, want, tag):
    print("%s status %d M %d/%d removed %d S %d/%d cand %d/%d outlier_ms %.2f" % (
        tag, j.status, j.num_points_processed, want["M"], j.num_outliers, j.num_samples_processed, want["S"], j.num_candidates, want["n_cand"],
        j.outlier_ms))
    assert j.status == 0, tag
    assert j.num_points_processed == want["M"] and j.num_outliers == want["voxelised"] - want["M"], tag
    assert j.num_samples_processed == want["S"] and j.num_candidates == want["n_cand"] == j.num_hands, tag
    if want["si"] is not None:
        assert np.array_equal(keep[7][: j.num_samples_processed], want["si"]), tag
    assert keep[5][: j.num_hands].tobytes() == want["records"].tobytes(), tag


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(api.default_params(15))
    c.set_lenet_weights(synth.lenet_weights(15, real=dict(np.load(os.path.join(GOLD, "lenet15_params.npz"))), trained_magnitude=True))
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(ctx):
    """(spec, stepwise result): coordinates route with the step on, the same scan with it off, index route with the step on"""
    a, sm_a = scan_with_flying_pixels(810, 40000)
    b, sm_b = scan_with_flying_pixels(820, 30000)
    specs = [(a, sm_a, 50, 1.0, 0, 0), (a, sm_a, 0, 0.0, 0, 0), (b, None, 50, 1.0, 60, 5), (b, sm_b, 20, 2.5, 0, 0)]
    return [(s, stepwise(ctx, *s)) for s in specs]


def test_step_alone_equals_the_stepwise_route(ctx, cases):
    (s_on, w_on), (s_off, w_off) = cases[0], cases[1]
    assert 40 <= w_on["voxelised"] - w_on["M"] < w_on["voxelised"] // 3 and w_on["n_cand"] > 50
    assert w_off["M"] == w_off["voxelised"] == w_on["voxelised"]
    assert w_on["records"].tobytes() != w_off["records"].tobytes()  # the step reaches the records
    jobs, keeps = build(ctx, [s_on])
    run(ctx, jobs)
    check(jobs[0], keeps[0], w_on, "alone")
    jobs, keeps = build(ctx, [cases[2][0]])
    run(ctx, jobs)
    check(jobs[0], keeps[0], cases[2][1], "alone, index route")
    assert cases[2][1]["si"].max() < cases[2][1]["M"]


def test_mixed_with_jobs_that_have_the_step_off_on_both_lanes(ctx, cases):
    order = [0, 1, 1, 2, 3, 0, 1, 3]  # lane 0: jobs 0, 2, 4, 6 — on, off, on, off; lane 1: off, on, on, on
    jobs, keeps = build(ctx, [cases[i][0] for i in order])
    run(ctx, jobs)
    for n, i in enumerate(order):
        check(jobs[n], keeps[n], cases[i][1], "mixed %d" % n)
    first = [k[5][: j.num_hands].tobytes() for j, k in zip(jobs, keeps)]
    run(ctx, jobs)
    assert [k[5][: j.num_hands].tobytes() for j, k in zip(jobs, keeps)] == first


def test_zeroed_fields_equal_the_job_without_them(ctx, cases):
    scan, sm = cases[1][0][0], cases[1][0][1]
    old, keep_old = ctx.raw_batch([scan], [sm], WS, CELL, RADIUS)
    assert old[0].outlier_mean_k == 0 and old[0].outlier_stddev_mult == 1.0
    old[0].outlier_stddev_mult = 0.0  # a zeroed struct
    run(ctx, old)
    check(old[0], keep_old[0], cases[1][1], "zeroed")
    assert old[0].num_outliers == 0 and old[0].outlier_ms == 0.0
    old[0].outlier_stddev_mult = float("nan")  # not read while the step is off
    run(ctx, old)
    check(old[0], keep_old[0], cases[1][1], "off, NaN multiplier")


def test_a_job_outside_the_domain_fails_alone(ctx, cases):
    full = cases[0][0][0]
    few = np.flatnonzero(inside(full["xyz"], WS))[:30]  # thirty points survive the cut: fewer than mean_k + 1
    tiny = dict(xyz=np.ascontiguousarray(full["xyz"][few]), cam_source=np.ascontiguousarray(full["cam_source"][:, few]),
                view_points=full["view_points"])
    sm = cases[0][0][1]
    specs = [cases[0][0], (tiny, sm, 50, 1.0, 0, 0), cases[3][0], (cases[0][0][0], sm, -2, 1.0, 0, 0), (cases[0][0][0], sm, 256, 1.0, 0, 0),
             (cases[0][0][0], sm, 50, float("nan"), 0, 0), cases[2][0]]
    jobs, keeps = build(ctx, specs)
    run(ctx, jobs, expect_rc=-1)  # the first error of the batch: job 1, fewer than mean_k + 1 points after the voxeliser
    assert "needs 51 points" in api.lib().gpd_hip_last_error().decode()
    assert [j.status for j in jobs] == [0, -1, 0, -1, -3, -1, 0]
    for i in (1, 3, 4, 5):
        assert jobs[i].num_hands == 0 and jobs[i].num_candidates == 0
    check(jobs[0], keeps[0], cases[0][1], "before the errors")
    check(jobs[2], keeps[2], cases[3][1], "between the errors")
    check(jobs[6], keeps[6], cases[2][1], "after the errors")
