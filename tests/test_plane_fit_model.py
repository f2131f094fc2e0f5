"""The host model of Cloud::sampleAbovePlane (util::Cloud::sampleAbovePlane -> gpd_host_sample_above_plane,
hostlib.sample_above_plane) against an independent numpy restatement (tests/pyref_plane.py), bit for bit:
indices off the plane, coefficient bits, inlier count, iterations.  No GPU."""
import numpy as np
import pytest

import pyref_plane as R
from gpd_amd import hostlib


def _same(xyz, **kw):
    want = R.fit(xyz, **kw)
    got = hostlib.sample_above_plane(xyz, **kw)
    assert np.array_equal(got[0], want[0])
    assert got[1].view(np.uint32).tolist() == want[1].view(np.uint32).tolist(), (got[1], want[1])
    assert got[2:] == want[2:], (got[2:], want[2:])
    return got


def test_mt19937_known_answers():
    r = R.Rnd(5489)
    for _ in range(9999):
        r.raw()
    assert r.raw() == 4123659995
    r = R.Rnd(12345)
    assert [r.raw() for _ in range(3)] == [3992670690, 3823185381, 1358822685]


@pytest.mark.parametrize("chunk", range(8))
def test_fuzz_scenes_equal_the_restatement(chunk):
    sc = R.scenes()
    assert len(sc) >= 300
    for name, xyz, kw in sc[chunk::8]:
        try:
            _same(xyz, **kw)
        except AssertionError as e:
            raise AssertionError("%s %s: %s" % (name, kw, e))


def test_scene_kinds_cover_success_and_failure():
    fails = ok = 0
    for name, xyz, kw in R.scenes():
        idx, c, inl, its = hostlib.sample_above_plane(xyz, **kw)
        if len(idx):
            ok += 1
            assert np.all(np.diff(idx) > 0) and inl + len(idx) == len(xyz)
        else:
            fails += 1
    assert ok > 250 and fails > 5


def test_small_clouds_fail():
    for n in range(3):
        idx, c, inl, its = hostlib.sample_above_plane(np.ones((n, 3), np.float32))
        assert len(idx) == 0 and its == 0 and not c.any()
    idx, c, inl, its = _same(np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32))  # collinear: no good sample
    assert len(idx) == 0 and its == 0


def test_zero_normal_draw_counts_every_point():
    """p2 == p0 with a zero component of p1 - p0 passes the good-sample test with a zero normal: plane (0, 0, 0, -0)
    whose distance is 0 for every point, so every point is an inlier and the fit "fails" (no point above it)."""
    p0, p1 = np.array([0, 0, 0], np.float32), np.array([1, 0, 2], np.float32)
    assert R.sample_good(p0, p1, p0)
    c = R.plane_from3(p0, p1, p0)
    assert not c[:3].any()
    xyz = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 2], [0, 0, 0], [1, 0, 2], [0, 0, 0], [3, 0, 5]], np.float32)
    idx, c, inl, its = _same(xyz, optimize=False)
    assert inl == len(xyz) and len(idx) == 0


def test_plane_is_found_and_samples_lie_off_it():
    rng = np.random.default_rng(3)
    xyz = R.table_scene(rng, 3000, 800, noise=0.001)
    idx, c, inl, its = _same(xyz)
    assert inl >= 3000 * 0.95 and len(idx) > 0
    d = np.abs((c[0] * xyz[idx, 0] + c[2] * xyz[idx, 2]) + (c[1] * xyz[idx, 1] + c[3]))
    assert (d.astype(np.float64) >= 0.01).all()


def test_table_mug_host_model():
    import os
    xyz = np.load(os.path.join(os.path.dirname(__file__), "golden", "table_mug_xyz.npz"))["xyz"]
    idx, c, inl, its = _same(xyz)
    assert inl > 0.8 * len(xyz)  # the table: ~86 % of the raw scan within 1 cm of one plane


def test_float_threshold_decides_like_the_double_compare():
    """The device tests fabsf(dist) <= threshold_f32(threshold) instead of (double)fabsf(dist) < threshold: the same
    decision for every float near the threshold (and both sides monotone), for the reference's 0.01 and the variants."""
    for t in (0.01, 0.005, 0.02, 0.0101, 0.0, 1e-3, 0.1, float(np.float32(0.01))):
        tf = R.threshold_f32(t)
        f = np.float32(abs(t))
        near = [f]
        up = dn = f
        for _ in range(64):
            up = np.nextafter(up, np.float32(np.inf))
            dn = np.nextafter(dn, np.float32(0))
            near += [up, dn]
        for v in near:
            assert (float(v) < t) == bool(v <= tf), (t, v, tf)
    assert R.threshold_f32(0.01) == np.float32(0.01)  # 0.01f lies below 0.01: `<= 0.01f`
