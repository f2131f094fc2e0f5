"""Cloud::refineNormals on the device (gpd_hip_refine_normals) equals the host model (util::Cloud::refineNormals,
hostlib.refine_normals) bit for bit: the refined normal bits with their NaN positions, the passes run, every mean of the
stop rule, the non-finite count — on the cases of tests/test_refine_normals_model.py, table_mug raw and voxelised after
estimate_normals on the device, the config-4 300k cloud and k = K_CAP; then a detect that follows without a re-upload
equals the oracle's detect on the refined normals, and GraspDetector::refineNormals equals the API."""
import os

import numpy as np
import pytest

import test_refine_normals_model as M
from gpd_amd import api, hostlib, synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
K_CAP = 256


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(api.default_params(15))
    yield c
    c.close()


def _same(dev, host):
    M.assert_same_normals(dev[0], host[0])
    assert dev[1] == host[1], (dev[1], host[1])
    assert dev[2].view(np.uint32).tolist() == host[2].view(np.uint32).tolist(), (dev[2], host[2])
    assert dev[3] == host[3]


def _both(ctx, xyz, nrm, k, **kw):
    xyz = np.ascontiguousarray(xyz, np.float32)
    nrm = np.ascontiguousarray(nrm, np.float32)
    ctx.upload_cloud(xyz, nrm)
    dev = ctx.refine_normals(k, **kw)
    host = hostlib.refine_normals(xyz, nrm, k, **kw)
    _same(dev, host)
    return dev


def _table_mug():
    return np.load(os.path.join(GOLD, "table_mug_xyz.npz"))["xyz"]


@pytest.mark.parametrize("kind", ["lattice", "off_lattice", "duplicated", "nan_normals"])
def test_model_cases(ctx, kind):
    xyz, nrm = {"lattice": M.lattice, "off_lattice": M.off_lattice, "duplicated": M.duplicated, "nan_normals": M.with_nan_normals}[kind]()
    for k in (1, 2, 10, 30, 50):
        for kw in ({}, {"convergence_threshold": 0.0}, {"max_iterations": 0}, {"max_iterations": 1}):
            _both(ctx, xyz, nrm, k, **kw)


def test_krylon_antipodal_and_small_clouds(ctx, oracle_mod):
    xyz, nrm = M.krylon(oracle_mod)
    for k in (10, 30):
        _both(ctx, xyz, nrm, k)
    pair = np.array([[0, 0, 0], [0.001, 0, 0]], np.float32)
    out, its, dd, nan = _both(ctx, pair, np.array([[0, 0, 1], [0, 0, -1]], np.float32), 2)
    assert nan == 2 and its == 15
    xyz, nrm = M.off_lattice(4000, 9)
    _both(ctx, xyz[:40], nrm[:40], 50)  # k > N: clamped
    _both(ctx, xyz[:1], nrm[:1], 5)
    _both(ctx, xyz, nrm, 10, convergence_threshold=0.5)


def test_table_mug_raw_and_voxelised_after_estimate_normals(ctx):
    raw = _table_mug()
    vox, _, _, _ = ctx.preprocess_cloud(raw, voxel_size=0.003)
    for xyz in (raw, vox):
        ctx.upload_cloud(xyz, np.zeros_like(xyz))
        est = ctx.estimate_normals(0.03)
        for k in (10, 30):
            dev = ctx.refine_normals(k)  # on the estimated normals, never re-uploaded
            host = hostlib.refine_normals(xyz, est, k)
            _same(dev, host)
            ctx.upload_cloud(xyz, est)  # back to the estimated normals for the next k
        print("table_mug %d points: kernel ms (kNN, passes, call) %s" % (len(xyz), ctx.last_refine_ms))


def test_config4_300k_at_k30(ctx):
    cl = synth.make_cloud(1234, 300000, clutter=True)
    dev = _both(ctx, cl["xyz"], cl["normals"], 30)
    assert dev[3] == 0
    print("300k: kernel ms (kNN, passes, call) %s, passes %d" % (ctx.last_refine_ms, dev[1]))


def test_k_cap_works_and_beyond_is_refused(ctx):
    vox, _, _, _ = ctx.preprocess_cloud(_table_mug(), voxel_size=0.003)
    nrm = np.zeros_like(vox)
    nrm[:, 2] = 1
    nrm += np.random.RandomState(3).randn(*nrm.shape).astype(np.float32) * np.float32(0.2)
    _both(ctx, vox, nrm, K_CAP, max_iterations=3)
    ctx.upload_cloud(vox, nrm)
    with pytest.raises(api.GpdHipError, match="capacity is 256"):
        ctx.refine_normals(K_CAP + 1)
    with pytest.raises(api.GpdHipError):
        ctx.refine_normals(0)
    _both(ctx, vox, nrm, 30)  # the context still works


def test_dense_sparse_dense_and_repeat(ctx):
    raw = _table_mug()
    est_ctx = api.Context(api.default_params(15))
    try:
        est_ctx.upload_cloud(raw, np.zeros_like(raw))
        est = est_ctx.estimate_normals(0.03)
    finally:
        est_ctx.close()
    first = _both(ctx, raw, est, 30)
    rng = np.random.RandomState(8)
    sparse = (rng.rand(300, 3) * 2 - 1).astype(np.float32)
    sn = rng.randn(300, 3).astype(np.float32)
    _both(ctx, sparse, sn, 50)
    _both(ctx, sparse, sn, 3, convergence_threshold=0.0)
    again = _both(ctx, raw, est, 30)
    _same(again, first)  # a repeated call gives the same bits


def test_detect_after_refine_uses_the_refined_normals(ctx, oracle_mod, lenet15_real):
    """preprocessPointCloud's order: normals, refineNormals, then the search — a detect right after the refinement (no
    re-upload) equals the oracle's detect on the refined normals."""
    import oracle
    vox, _, _, _ = ctx.preprocess_cloud(_table_mug(), voxel_size=0.003)
    cam = np.ones((1, len(vox)), np.int32)
    vp = np.zeros((1, 3), np.float64)
    ctx.set_lenet_weights(lenet15_real)
    ctx.upload_cloud(vox, np.zeros_like(vox), cam, vp)
    est = ctx.estimate_normals(0.03)
    refined, its, dd, nan = ctx.refine_normals(20)
    assert nan == 0 and its >= 1
    assert not np.array_equal(refined, est)
    si = np.ascontiguousarray(np.random.RandomState(5).permutation(len(vox))[:24], np.int32)
    hands, n_cand = ctx.detect(si)
    p = oracle.default_params(15)
    ohands, on_cand, _ = oracle.detect(p, vox, refined, cam, vp, si, lenet15_real)
    assert n_cand == on_cand and n_cand > 0
    assert np.array_equal(hands["valid"], ohands["valid"])
    v = ohands["valid"].astype(bool)
    assert np.array_equal(hands["finger_placement_index"][v], ohands["finger_placement_index"][v])
    assert float(np.abs(hands["score"][v] - ohands["score"][v]).max()) <= 1e-4
    # ... and differs from the detect on the unrefined normals somewhere (the refinement reached the search)
    ehands, _, _ = oracle.detect(p, vox, est, cam, vp, si, lenet15_real)
    assert len(ehands) != len(ohands) or ehands.tobytes() != ohands.tobytes()


def test_grasp_detector_refine_normals_equals_the_api(ctx):
    xyz, nrm = M.off_lattice(6000, 12)
    ctx.upload_cloud(xyz, nrm)
    dev = ctx.refine_normals(30)
    mirror = hostlib.detector_refine_normals(xyz, nrm, 30)
    M.assert_same_normals(mirror, dev[0])
