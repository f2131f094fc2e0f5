"""The host model of Cloud::removeStatisticalOutliers (gpd_amd/csrc/outlier_model.h through hostlib.remove_statistical_outliers;
DESIGN §7) against an independent numpy restatement (tests/pyref_outliers.py), bit for bit: the kept indices, the bits of every
point's mean neighbour distance and of the three statistics.  Then the mirror's util::Cloud::removeStatisticalOutliers (normals,
camera columns and sample indices follow the points) and the refusals that need no device.  No GPU."""
import ctypes

import numpy as np
import pytest

import pyref_outliers as R
from gpd_amd import hostlib, synth

# lattice_equal(seed): the seed whose variance comes out negative (a NaN threshold) and one whose variance is positive; found by
# running lattice_equal over seeds 0 .. 19 on the restatement (the sign is that of fl32(h * h) - h * h, a coin per seed)
SEED_NAN, SEED_POSITIVE = 1, 0


def lattice_equal(seed):
    """A shuffled box lattice whose every point has its three nearest neighbours at the same float distance: the spacing h is
    a float of 16 significant bits and the indices stay below 256, so every coordinate i * h and every difference is exact,
    d2 = fl32(h * h) and sqrtf gives h back.  With mean_k <= 3 all mean distances equal h; the variance is then pure rounding,
    (n fl32(h h) - fl64(fl64(n n h h) / n)) / (n - 1), of either sign."""
    rng = np.random.RandomState(seed)
    h = np.float32(int(rng.randint(1 << 15, 1 << 16) | 1) * 2.0 ** -24)  # 0.002 .. 0.004
    dims = rng.randint(6, 13, 3)
    org = rng.randint(0, 100, 3)
    g = np.stack(np.meshgrid(*[np.arange(o, o + d) for o, d in zip(org, dims)], indexing="ij"), -1).reshape(-1, 3)
    xyz = g.astype(np.float32) * h
    assert np.array_equal(xyz.astype(np.float64), g * np.float64(h))  # exact
    return xyz[rng.permutation(len(xyz))], h


def off_lattice(n=3000, seed=11):
    return synth.off_lattice(synth.make_cloud(seed, n))["xyz"]


def duplicated():
    xyz = off_lattice(1500, 3)
    rng = np.random.RandomState(4)
    pick = rng.randint(0, len(xyz), 700)
    xyz = np.concatenate([xyz, xyz[pick], xyz[pick[:100]]])
    return xyz[rng.permutation(len(xyz))]


def planted():
    """a 3000-point off-lattice surface and 20 isolated points 0.3 m and more above it, 0.3 m apart -> (xyz, planted indices)"""
    surf = off_lattice(3000, 5)
    rng = np.random.RandomState(8)
    hi = surf.max(0)
    iso = np.array([[hi[0] - 0.3 * (i % 5), hi[1] - 0.3 * (i // 5), hi[2] + 0.3 + 0.01 * i] for i in range(20)])
    iso = (iso + rng.uniform(-0.01, 0.01, iso.shape)).astype(np.float32)
    xyz = np.concatenate([surf, iso])
    perm = rng.permutation(len(xyz))
    where = np.sort(np.argsort(perm)[len(surf):]).astype(np.int32)  # perm[where] >= len(surf)
    return np.ascontiguousarray(xyz[perm]), where


_D2 = {}


def reference(name, xyz, mean_k, mult):
    """the restatement, its d2 matrix computed once per cloud"""
    key = (name, len(xyz))
    ranks = min(len(xyz), 256)
    if key not in _D2:
        _D2[key] = R.sorted_d2(xyz, ranks)
    return R.remove_statistical_outliers(xyz, mean_k, mult, _D2[key])


def assert_same(got, want):
    kept, stats, dist = got
    assert np.array_equal(dist.view(np.uint32), want[2].view(np.uint32)), np.flatnonzero(dist.view(np.uint32) != want[2].view(np.uint32))[:5]
    assert stats.view(np.uint64).tolist() == want[1].view(np.uint64).tolist(), (stats, want[1])
    assert np.array_equal(kept, want[0])
    assert (np.diff(kept) > 0).all()


def same(name, xyz, mean_k, mult):
    want = reference(name, xyz, mean_k, mult)
    got = hostlib.remove_statistical_outliers(xyz, mean_k, mult)
    assert_same(got, want)
    return got, want


CLOUDS = {"off_lattice": off_lattice, "duplicated": duplicated, "planted": lambda: planted()[0]}


@pytest.mark.parametrize("kind", sorted(CLOUDS))
@pytest.mark.parametrize("mean_k", [1, 2, 50, 255])
def test_model_equals_the_restatement(kind, mean_k):
    xyz = CLOUDS[kind]()
    for mult in (0.0, 1.0, 2.5, -1.0):
        (kept, stats, dist), _ = same(kind, xyz, mean_k, mult)
        # (mult = -1 on the duplicated cloud at mean_k = 1: the zeros make stddev > mean, the threshold negative, and no point is kept)
        assert len(kept) > 0 or (mult < 0 and stats[2] < 0)
        if mult >= 1.0:
            assert len(kept) < len(xyz)  # something is removed: the clouds are no lattices
    if kind == "duplicated" and mean_k == 1:
        assert (dist == 0).sum() >= 700  # a twin at d2 = 0 is rank 1


def test_equal_distances_keep_everything_also_under_a_nan_threshold():
    seen_nan = False
    for seed in (SEED_NAN, SEED_POSITIVE):
        xyz, h = lattice_equal(seed)
        for mean_k in (1, 2, 3):
            for mult in (1.0, 0.0, -1.0):
                (kept, stats, dist), want = same("lattice%d" % seed, xyz, mean_k, mult)
                assert (dist == h).all()
                assert len(kept) == len(xyz) or (mult < 0 and stats[1] > 0)
                if seed == SEED_NAN:
                    assert want[3] < 0 and np.isnan(stats[1]) and np.isnan(stats[2]) and len(kept) == len(xyz)
                    seen_nan = True
                elif mean_k == 1:
                    assert want[3] > 0 and stats[2] == stats[0] + mult * stats[1]
    assert seen_nan


def test_planted_isolated_points_are_removed():
    xyz, where = planted()
    want = reference("planted", xyz, 50, 1.0)
    assert not np.isin(where, want[0]).any()  # the restatement removes all twenty ...
    (kept, stats, dist), _ = same("planted", xyz, 50, 1.0)
    assert not np.isin(where, kept).any()  # ... and so does the model
    assert (np.diff(kept) > 0).all()
    assert dist[where].min() > stats[2] > np.median(dist)
    assert len(xyz) - len(kept) < 0.2 * len(xyz)


def test_smallest_clouds_of_the_domain():
    xyz = off_lattice(3000, 9)
    for mean_k in (1, 2, 50, 255):
        sub = np.ascontiguousarray(xyz[: mean_k + 1])
        for mult in (0.0, 1.0):
            same("head%d" % mean_k, sub, mean_k, mult)  # N == mean_k + 1: every list is the whole cloud
    for n, mean_k in ((63, 10), (64, 50), (65, 64), (257, 255)):
        same("n%d" % n, np.ascontiguousarray(xyz[:n]), mean_k, 1.0)


def test_refusals():
    xyz = off_lattice(3000, 9)
    with pytest.raises(ValueError):
        hostlib.remove_statistical_outliers(xyz[:50], 50, 1.0)  # N = mean_k
    with pytest.raises(ValueError):
        hostlib.remove_statistical_outliers(xyz, 0, 1.0)
    with pytest.raises(ValueError):
        hostlib.remove_statistical_outliers(xyz, -5, 1.0)
    with pytest.raises(ValueError):
        hostlib.remove_statistical_outliers(xyz, 50, float("nan"))
    with pytest.raises(ValueError):
        hostlib.remove_statistical_outliers(xyz, 50, float("inf"))
    with pytest.raises(OverflowError):
        hostlib.remove_statistical_outliers(xyz, 256, 1.0)
    kept, _, _ = hostlib.remove_statistical_outliers(xyz[:51], 50, 1.0)  # the edge itself is inside
    assert len(kept) > 0


def test_capi_refuses_bad_arguments_without_a_device():
    """gpd_hip_remove_statistical_outliers checks its arguments before it touches a context or the device: a null context or
    output, mean_k < 1 or a non-finite multiplier is GPD_ERR_INVALID; mean_k beyond the capacity GPD_ERR_CAPACITY."""
    from gpd_amd import api
    L = api.lib()
    kept = (ctypes.c_int32 * 8)()
    stats = (ctypes.c_double * 3)()
    num = ctypes.c_int(0)
    not_a_context = ctypes.create_string_buffer(64)  # never dereferenced: every call below is refused first

    def call(ctx, mean_k=50, mult=1.0, k=kept, n=ctypes.byref(num), s=stats):
        return L.gpd_hip_remove_statistical_outliers(ctx, mean_k, ctypes.c_double(mult), k, n, s, None, None)

    assert call(None) == -1
    assert call(not_a_context, k=None) == -1
    assert call(not_a_context, n=None) == -1
    assert call(not_a_context, s=None) == -1
    assert call(not_a_context, mean_k=0) == -1
    assert call(not_a_context, mean_k=-1) == -1
    assert call(not_a_context, mult=float("nan")) == -1
    assert call(not_a_context, mult=float("-inf")) == -1
    assert b"bad argument" in L.gpd_hip_last_error()
    assert call(not_a_context, mean_k=256) == -3
    assert b"capacity is 255" in L.gpd_hip_last_error()


def test_detect_job_mirror_has_the_outlier_fields_at_the_end():
    from gpd_amd import api
    names = [f[0] for f in api.DetectJob._fields_]
    assert names[-5:] == ["outlier_mean_k", "num_outliers", "outlier_stddev_mult", "outlier_ms", "reserved2_"]
    j = api.DetectJob()
    assert j.outlier_mean_k == 0 and j.outlier_stddev_mult == 0.0  # a zeroed struct: the step is off


def test_mirror_cloud_carries_normals_cameras_and_remaps_samples():
    """util::Cloud::removeStatisticalOutliers on a two-camera cloud: normals and camera columns follow their points, sample
    indices are remapped to the kept cloud, those of removed points dropped, order (and repetitions) kept."""
    xyz, where = planted()
    n = len(xyz)
    rng = np.random.RandomState(12)
    nrm = rng.randn(n, 3).astype(np.float32)
    cam = rng.randint(0, 2, (2, n)).astype(np.int32)
    kept, _, _ = hostlib.remove_statistical_outliers(xyz, 50, 1.0)
    removed = np.setdiff1d(np.arange(n), kept)
    assert len(removed) >= 20
    samples = np.concatenate([rng.randint(0, n, 200), removed[:15], kept[:5], kept[:5], where[:3]]).astype(np.int32)
    samples = samples[rng.permutation(len(samples))]
    xo, no, co, so = hostlib.cloud_remove_statistical_outliers(xyz, nrm, cam, samples, 50, 1.0)
    assert np.array_equal(xo.view(np.uint32), xyz[kept].view(np.uint32))
    assert np.array_equal(no.view(np.uint32), nrm[kept].view(np.uint32))
    assert np.array_equal(co, cam[:, kept])
    new_index = np.full(n, -1)
    new_index[kept] = np.arange(len(kept))
    want = new_index[samples]
    want = want[want >= 0]
    assert 0 < len(want) < len(samples)
    assert np.array_equal(so, want)
    assert np.array_equal(xo[so], xyz[samples[new_index[samples] >= 0]])  # every surviving sample still names its point
    # a cloud without normals stays without
    xo2, no2, co2, so2 = hostlib.cloud_remove_statistical_outliers(xyz, None, cam, samples, 50, 1.0)
    assert no2 is None and np.array_equal(xo2, xo) and np.array_equal(co2, co) and np.array_equal(so2, so)
    with pytest.raises(ValueError):
        hostlib.cloud_remove_statistical_outliers(xyz[:50], None, cam[:, :50], samples[:0], 50, 1.0)
