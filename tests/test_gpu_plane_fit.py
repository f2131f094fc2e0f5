"""Cloud::sampleAbovePlane on the device (gpd_hip_sample_above_plane) equals the host model
(util::Cloud::sampleAbovePlane, hostlib.sample_above_plane) bit for bit: indices off the plane, the plane's coefficient
bits, the inlier count, the iterations — on table_mug raw and voxelised, krylon, the config-4 300k cloud and the fuzz
scenes of tests/pyref_plane.py; then a detect at the sampled indices equals the oracle's."""
import os

import numpy as np
import pytest

import pyref_plane
from gpd_amd import api, hostlib, synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(api.default_params(15))
    yield c
    c.close()


def _fit_both(ctx, xyz, **kw):
    xyz = np.ascontiguousarray(xyz, np.float32)
    ctx.upload_cloud(xyz, np.zeros_like(xyz))
    dev = ctx.sample_above_plane(**kw)
    host = hostlib.sample_above_plane(xyz, **kw)
    assert np.array_equal(dev[0], host[0])
    assert dev[1].view(np.uint32).tolist() == host[1].view(np.uint32).tolist(), (dev[1], host[1])
    assert dev[2:] == host[2:]
    return dev


def _table_mug():
    return np.load(os.path.join(GOLD, "table_mug_xyz.npz"))["xyz"]


def test_table_mug_raw(ctx):
    xyz = _table_mug()
    idx, c, inl, its = _fit_both(ctx, xyz)
    assert inl > 0.8 * len(xyz)  # the table
    assert len(idx) == len(xyz) - inl and len(idx) > 0


def test_table_mug_voxelised(ctx):
    vox, _, _, _ = ctx.preprocess_cloud(_table_mug(), voxel_size=0.003)
    idx, c, inl, its = _fit_both(ctx, vox)
    assert inl > 0.5 * len(vox) and len(idx) > 0


def test_krylon_and_config4(ctx):
    kr = np.load(os.path.join(GOLD, "krylon_xyz.npz"))
    _fit_both(ctx, kr[list(kr.keys())[0]])
    big = synth.make_cloud(1234, 300000, clutter=True)["xyz"]
    idx, c, inl, its = _fit_both(ctx, big)
    assert len(idx) > 0


def test_parameter_variants_on_table_mug(ctx):
    vox, _, _, _ = ctx.preprocess_cloud(_table_mug(), voxel_size=0.003)
    for kw in ({"threshold": 0.005}, {"threshold": 0.0}, {"max_iterations": 0}, {"max_iterations": 200, "probability": 0.9999},
               {"optimize": False}):
        _fit_both(ctx, vox, **kw)


def test_fuzz_scenes(ctx):
    for name, xyz, kw in pyref_plane.scenes():
        if len(xyz) == 0:
            continue  # a context takes no empty cloud
        try:
            _fit_both(ctx, xyz, **kw)
        except AssertionError as e:
            raise AssertionError("%s %s: %s" % (name, kw, e))


def test_capacity_is_refused(ctx):
    xyz = _table_mug()[:1000]
    ctx.upload_cloud(xyz, np.zeros_like(xyz))
    with pytest.raises(api.GpdHipError):
        ctx.sample_above_plane(max_iterations=5000)


def test_detect_at_the_samples_above_the_plane(ctx, oracle_mod, lenet15_real):
    """ur5.cfg's order: normals, sampleAbovePlane, subsample; the detect at those samples equals the oracle's."""
    import oracle
    vox, _, _, _ = ctx.preprocess_cloud(_table_mug(), voxel_size=0.003)
    cam = np.ones((1, len(vox)), np.int32)
    vp = np.zeros((1, 3), np.float64)
    ctx.upload_cloud(vox, np.zeros_like(vox), cam, vp)
    normals = ctx.estimate_normals(0.03)
    idx, c, inl, its = ctx.sample_above_plane()
    assert len(idx) > 100
    dist = np.abs((c[0] * vox[idx, 0] + c[2] * vox[idx, 2]) + (c[1] * vox[idx, 1] + c[3]))
    assert (dist.astype(np.float64) >= 0.01).all()  # no sample lies on the plane
    si = np.ascontiguousarray(idx[np.random.RandomState(5).permutation(len(idx))[:24]], np.int32)
    ctx.set_lenet_weights(lenet15_real)
    ctx.upload_cloud(vox, normals, cam, vp)
    hands, n_cand = ctx.detect(si)
    p = oracle.default_params(15)
    ohands, on_cand, _ = oracle.detect(p, vox, normals, cam, vp, si, lenet15_real)
    assert n_cand == on_cand and n_cand > 0
    assert np.array_equal(hands["valid"], ohands["valid"])
    v = ohands["valid"].astype(bool)
    assert np.array_equal(hands["finger_placement_index"][v], ohands["finger_placement_index"][v])
    assert float(np.abs(hands["score"][v] - ohands["score"][v]).max()) <= 1e-4
