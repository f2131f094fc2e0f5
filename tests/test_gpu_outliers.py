"""Cloud::removeStatisticalOutliers on the device (gpd_hip_remove_statistical_outliers) equals the host model
(gpd_amd/csrc/outlier_model.h, hostlib.remove_statistical_outliers) bit for bit: the kept indices, every point's mean neighbour
distance, the three statistics — on the cases of tests/test_outlier_model.py, clouds around the wave size, a grid of one cell
and table_mug voxelised; then what the call leaves on the device: a detect on the resident cloud equals a detect on the uploaded
kept points, normals and camera rows follow their points, refusals leave the cloud alone, and refine_normals (which shares the
search) still equals its host model."""
import os

import numpy as np
import pytest

import test_outlier_model as M
import test_refine_normals_model as RM
from gpd_amd import api, hostlib, synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(api.default_params(15))
    c.set_lenet_weights(synth.lenet_weights(15, real=dict(np.load(os.path.join(GOLD, "lenet15_params.npz"))), trained_magnitude=True))
    yield c
    c.close()


def _both(ctx, xyz, mean_k, mult):
    """upload, filter on the device, filter on the host: equal; a filter that keeps nothing is refused and changes nothing"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    host = hostlib.remove_statistical_outliers(xyz, mean_k, mult)
    ctx.upload_cloud(xyz, np.zeros_like(xyz))
    if len(host[0]) == 0:
        with pytest.raises(api.GpdHipError, match="no point is left"):
            ctx.remove_statistical_outliers(mean_k, mult)
        assert ctx._num_points == len(xyz)
        return None
    dev = ctx.remove_statistical_outliers(mean_k, mult)
    M.assert_same(dev, host)
    assert ctx._num_points == len(host[0])
    return dev


@pytest.mark.parametrize("kind", sorted(M.CLOUDS))
def test_model_cases(ctx, kind):
    xyz = M.CLOUDS[kind]()
    for mean_k in (1, 2, 50, 255):
        for mult in (0.0, 1.0, 2.5, -1.0):
            _both(ctx, xyz, mean_k, mult)
    print("%s %d points: kernel ms (distances, compaction, call) %s" % (kind, len(xyz), ctx.last_outlier_ms))


def test_equal_distances_and_a_nan_threshold_keep_everything(ctx):
    for seed in (M.SEED_NAN, M.SEED_POSITIVE):
        xyz, h = M.lattice_equal(seed)
        for mean_k in (1, 2, 3):
            for mult in (1.0, 0.0):
                kept, stats, dist = _both(ctx, xyz, mean_k, mult)
                assert len(kept) == len(xyz) and (dist == h).all()
                assert np.isnan(stats[2]) == (seed == M.SEED_NAN)


def test_planted_points_leave(ctx):
    xyz, where = M.planted()
    kept, stats, dist = _both(ctx, xyz, 50, 1.0)
    assert not np.isin(where, kept).any() and (np.diff(kept) > 0).all()


@pytest.mark.parametrize("n,mean_k", [(2, 1), (51, 50), (51, 7), (63, 62), (63, 10), (64, 63), (64, 50), (65, 64), (65, 1), (256, 255),
                                      (257, 255), (257, 64)])
def test_sizes_around_the_wave(ctx, n, mean_k):
    xyz = M.off_lattice(3000, 9)[:n]
    for mult in (0.0, 1.0):
        _both(ctx, xyz, mean_k, mult)


def test_grid_of_one_cell(ctx):
    rng = np.random.RandomState(21)
    xyz = (np.array([0.3, -0.2, 0.7]) + rng.uniform(0, 0.015, (500, 3))).astype(np.float32)  # inside one 2 cm cell
    for mean_k in (1, 50, 255):
        _both(ctx, xyz, mean_k, 1.0)
    _both(ctx, xyz[:51], 50, 1.0)


def test_table_mug_voxelised(ctx):
    raw = np.load(os.path.join(GOLD, "table_mug_xyz.npz"))["xyz"]
    vox, _, _, _ = ctx.preprocess_cloud(raw, voxel_size=0.003)
    kept, stats, dist = _both(ctx, vox, 50, 1.0)
    assert 0 < len(vox) - len(kept) < 0.2 * len(vox)
    print("table_mug %d points, %d removed: kernel ms (distances, compaction, call) %s" % (len(vox), len(vox) - len(kept), ctx.last_outlier_ms))


def _scene():
    """a surface with analytic normals, two cameras with mixed flags, and planted isolated points"""
    c = synth.off_lattice(synth.make_cloud(31, 12000))
    rng = np.random.RandomState(32)
    hi = c["xyz"].max(0)
    iso = np.array([[hi[0] - 0.1 * (i % 5), hi[1] - 0.1 * (i // 5), hi[2] + 0.15 + 0.01 * i] for i in range(20)], np.float32)
    xyz = np.concatenate([c["xyz"], iso])
    nrm = np.concatenate([c["normals"], np.tile(np.array([[0, 0, 1]], np.float32), (20, 1))])
    perm = rng.permutation(len(xyz))
    xyz, nrm = np.ascontiguousarray(xyz[perm]), np.ascontiguousarray(nrm[perm])
    cam = rng.randint(0, 2, (2, len(xyz))).astype(np.int32)
    cam[0] |= 1 - cam[1]  # every point seen by a camera
    vp = np.array([[0.0, 0.0, 0.0], [0.1, -0.1, -1.6]])  # one camera above the table, one below: which one sees a point decides its normal's sign
    return xyz, nrm, cam, vp


def test_normals_and_camera_rows_follow_their_points(ctx):
    xyz, nrm, cam, vp = _scene()
    ctx.upload_cloud(xyz, nrm, cam, vp)
    kept, stats, dist = ctx.remove_statistical_outliers(50, 1.0)
    host = hostlib.remove_statistical_outliers(xyz, 50, 1.0)
    M.assert_same((kept, stats, dist), host)
    assert 20 <= len(xyz) - len(kept) < len(xyz) // 4
    # the device's normals, read back by a refinement of zero passes: numpy's gather
    resident = ctx.refine_normals(1, max_iterations=0)[0]
    assert np.array_equal(resident.view(np.uint32), nrm[kept].view(np.uint32))
    # a detect on the resident cloud is the detect on the gathered one
    si = np.ascontiguousarray(np.random.RandomState(33).permutation(len(kept))[:16], np.int32)
    hands, n_cand = ctx.detect(si)
    ctx.upload_cloud(xyz[kept], nrm[kept], cam[:, kept], vp)
    want, want_cand = ctx.detect(si)
    assert n_cand == want_cand > 0 and hands.tobytes() == want.tobytes()


def test_estimate_normals_and_detect_on_the_resident_cloud(ctx):
    xyz, _, cam, vp = _scene()
    ctx.upload_cloud(xyz, np.zeros_like(xyz), cam, vp)
    kept, _, _ = ctx.remove_statistical_outliers(50, 1.0)
    est = ctx.estimate_normals(0.03)
    si = np.ascontiguousarray(np.random.RandomState(34).permutation(len(kept))[:16], np.int32)
    hands, n_cand = ctx.detect(si)
    ctx.upload_cloud(xyz[kept], np.zeros((len(kept), 3), np.float32), cam[:, kept], vp)
    want_est = ctx.estimate_normals(0.03)
    want, want_cand = ctx.detect(si)
    # the normals point towards the cameras that see each point: equal normals say the camera rows followed their points ...
    assert est.shape == (len(kept), 3) and np.array_equal(est.view(np.uint32), want_est.view(np.uint32))
    assert n_cand == want_cand > 0 and hands.tobytes() == want.tobytes()
    ctx.upload_cloud(xyz[kept], np.zeros((len(kept), 3), np.float32), cam[::-1, kept], vp)
    swapped = ctx.estimate_normals(0.03)  # ... since other rows give other normals
    assert (np.abs(swapped - want_est).max(axis=1) > 0.5).sum() > len(kept) // 10


def test_refusals_leave_the_cloud_untouched(ctx):
    xyz, nrm, cam, vp = _scene()
    xyz, nrm, cam = xyz[:200], nrm[:200], cam[:, :200]
    big = synth.off_lattice(synth.make_cloud(35, 6000))
    ctx.upload_cloud(big["xyz"], big["normals"])
    si = np.ascontiguousarray(np.random.RandomState(36).permutation(len(big["xyz"]))[:12], np.int32)
    before, n_before = ctx.detect(si)
    for mean_k, mult, text in ((0, 1.0, "bad argument"), (-3, 1.0, "bad argument"), (256, 1.0, "capacity is 255"),
                               (50, float("nan"), "bad argument"), (50, float("inf"), "bad argument")):
        with pytest.raises(api.GpdHipError, match=text):
            ctx.remove_statistical_outliers(mean_k, mult)
    after, n_after = ctx.detect(si)
    assert n_before == n_after > 0 and before.tobytes() == after.tobytes() and ctx._num_points == len(big["xyz"])
    ctx.upload_cloud(xyz, nrm, cam, vp)
    with pytest.raises(api.GpdHipError, match="needs 201 points"):
        ctx.remove_statistical_outliers(200, 1.0)  # N = mean_k
    assert ctx._num_points == 200
    assert np.array_equal(ctx.refine_normals(1, max_iterations=0)[0].view(np.uint32), nrm.view(np.uint32))
    kept, _, _ = ctx.remove_statistical_outliers(199, 1.0)  # the edge works
    assert 0 < len(kept) <= 200
    fresh = api.Context(api.default_params(15))
    try:
        with pytest.raises(api.GpdHipError, match="no cloud"):
            fresh.remove_statistical_outliers(50, 1.0)
    finally:
        fresh.close()


def test_refine_normals_still_equals_its_host_model(ctx):
    """the shell search moved to a header both kernels include: knn_kernel's lists are unchanged"""
    xyz, nrm = RM.off_lattice()
    ctx.upload_cloud(xyz, nrm)
    ctx.remove_statistical_outliers(50, 3.0)  # the same search with another epilogue, on the same context, first
    xyz, nrm = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(nrm, np.float32)
    for k in (10, 50):
        ctx.upload_cloud(xyz, nrm)
        dev = ctx.refine_normals(k)
        host = hostlib.refine_normals(xyz, nrm, k)
        RM.assert_same_normals(dev[0], host[0])
        assert dev[1] == host[1] and dev[3] == host[3]
        assert dev[2].view(np.uint32).tolist() == host[2].view(np.uint32).tolist()


def test_grasp_detector_mirror_equals_the_api(ctx):
    xyz, nrm, _, _ = _scene()
    rng = np.random.RandomState(37)
    samples = rng.randint(0, len(xyz), 300).astype(np.int32)
    ctx.upload_cloud(xyz, nrm)
    kept, _, _ = ctx.remove_statistical_outliers(50, 1.0)
    xo, no, so = hostlib.detector_remove_statistical_outliers(xyz, nrm, samples, 50, 1.0)
    assert np.array_equal(xo.view(np.uint32), xyz[kept].view(np.uint32))
    assert np.array_equal(no.view(np.uint32), nrm[kept].view(np.uint32))
    new_index = np.full(len(xyz), -1)
    new_index[kept] = np.arange(len(kept))
    want = new_index[samples]
    assert np.array_equal(so, want[want >= 0])
