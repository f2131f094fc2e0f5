"""The seeded shadow jitter on the host, no GPU: gpd_hip_shadow_jitter_model (gpd_amd/csrc/jitter_model.h) against the numpy
statement of tests/pyref_jitter.py, the moments of the draw, and gpd_hip_image_model_jitter — the voxel windows the image stage
takes with the jitter on (gpd_amd/csrc/image_model.h image::window_class)."""
import ctypes as C
import math

import numpy as np
import pytest

import pyref_jitter as J
import ref_cases as rc
from gpd_amd import api

GPD_ERR_INVALID = -1
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
SEEDS = (0, 2 ** 64 - 1, 1, 0x9E3779B97F4A7C15, 12345678901234567)


def _edge_voxels():
    rng = np.random.RandomState(7)
    edge = [I32_MIN, I32_MIN + 1, -65537, -65536, -2, -1, 0, 1, 2, 65535, 65536, I32_MAX - 1, I32_MAX]
    grid = np.array([(x, y, z) for x in edge for y in edge for z in edge], np.int64)
    near = rng.randint(-400, 400, (4000, 3))
    wide = rng.randint(I32_MIN, I32_MAX, (4000, 3), dtype=np.int64)
    return np.concatenate([grid, near, wide]).astype(np.int32)


def test_exports():
    for name in ("gpd_hip_set_shadow_jitter", "gpd_hip_shadow_jitter_model", "gpd_hip_image_model_jitter"):
        assert name in api.EXPORTS and getattr(api.lib(), name)


@pytest.mark.parametrize("seed", SEEDS)
def test_model_equals_the_numpy_statement(seed):
    v = _edge_voxels()
    assert (v == 0).all(axis=1).any() and (v < 0).any() and (v == I32_MIN).any() and (v == I32_MAX).any()
    got = api.shadow_jitter_model(seed, v)
    want = J.draws(seed, v)
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
    assert (np.abs(got) < 6.0).all()
    # multiples of 2^-16: every step of the definition is exact
    assert np.array_equal(got * 65536.0, np.round(got * 65536.0))


def test_mix_is_splitmix64():
    """The first outputs of splitmix64 from state 0 (the published test vector of the generator): mix(k * gamma) for k = 0, 1, 2"""
    gamma = 0x9E3779B97F4A7C15
    z = np.array([(k * gamma) & (2 ** 64 - 1) for k in range(3)], np.uint64)
    assert [int(x) for x in J.mix(z)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def test_seeds_and_coordinates_all_matter():
    v = np.array([[3, -7, 11]], np.int32)
    base = api.shadow_jitter_model(5, v)[0]
    others = [api.shadow_jitter_model(6, v)[0]] + [api.shadow_jitter_model(5, v + np.eye(3, dtype=np.int32)[a])[0] for a in range(3)]
    others.append(api.shadow_jitter_model(5, v[:, [1, 0, 2]])[0])
    assert all(o != base for o in others), (base, others)


def test_bad_arguments():
    L = api.lib()
    v = np.zeros((1, 3), np.int32)
    g = np.zeros(1, np.float64)
    assert L.gpd_hip_shadow_jitter_model(0, None, 1, g.ctypes.data) == GPD_ERR_INVALID
    assert L.gpd_hip_shadow_jitter_model(0, v.ctypes.data, 1, None) == GPD_ERR_INVALID
    assert L.gpd_hip_shadow_jitter_model(0, v.ctypes.data, -1, g.ctypes.data) == GPD_ERR_INVALID
    assert b"gpd_hip_shadow_jitter_model" in L.gpd_hip_last_error()
    assert L.gpd_hip_shadow_jitter_model(0, v.ctypes.data, 0, g.ctypes.data) == 0
    assert len(api.shadow_jitter_model(3, np.zeros((0, 3), np.int32))) == 0
    # the setter without a context (its other refusals need a context: tests/test_gpu_shadow_jitter.py)
    assert L.gpd_hip_set_shadow_jitter(None, 1, 0) == GPD_ERR_INVALID
    assert b"gpd_hip_set_shadow_jitter" in L.gpd_hip_last_error()


def test_moments_over_a_block_with_negative_coordinates():
    """128^3 voxels.  The draw is Irwin-Hall with twelve terms: mean 0, variance 1 - 2^-32, fourth moment 2.9.  The bounds are
    five standard errors of the estimators for independent draws (sd of the mean 1 / sqrt(N); of the variance sqrt(2 / N),
    the normal value, above Irwin-Hall's sqrt(1.9 / N)) — from the distribution, not from a run."""
    ax = np.arange(-100, 28, dtype=np.int32)
    v = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    N = len(v)
    assert N == 128 ** 3
    g = api.shadow_jitter_model(42, v)
    assert (np.abs(g) < 6.0).all()
    mean, var = float(g.mean()), float(g.var())
    print("mean %.3e (bound %.3e)  variance - 1 %.3e (bound %.3e)  fourth moment %.4f" %
          (mean, 5 / math.sqrt(N), var - 1, 5 * math.sqrt(2 / N), float((g ** 4).mean())))
    assert abs(mean) <= 5.0 / math.sqrt(N)
    assert abs(var - 1.0) <= 5.0 * math.sqrt(2.0 / N)
    # neighbours along each axis and a second seed: uncorrelated (|r| of independent draws: sd 1 / sqrt(N), five of them)
    cube = g.reshape(128, 128, 128)
    for a in range(3):
        lo = np.take(cube, np.arange(127), axis=a).ravel()
        hi = np.take(cube, np.arange(1, 128), axis=a).ravel()
        assert abs(float(np.corrcoef(lo, hi)[0, 1])) <= 5.0 / math.sqrt(len(lo)), a
    assert abs(float(np.corrcoef(g, api.shadow_jitter_model(43, v))[0, 1])) <= 5.0 / math.sqrt(N)


def test_restatement_draws_the_voxels_of_pyref():
    """tests/pyref_jitter.py draws a set's shadow voxels on arrays: the same voxels as pyref's loop, and the same draws consumed"""
    import pyref
    rng = np.random.RandomState(2)
    pts = (rng.uniform(-0.05, 0.05, (60, 3)) + np.array([0.1, -0.2, 0.7])).astype(np.float32)
    a, b = pyref.Lcg(0), pyref.Lcg(0)
    for vp in ([0.0, 0.0, 0.0], [0.3, -0.2, 0.1]):
        assert J.shadow_voxels(pts, vp, a) == pyref.shadow_voxels(pts, vp, b) and a.s == b.s
    cams = np.array([[1] * 60, [0] * 59 + [1]])
    vps = np.array([[0.0, 0.0, 0.0], [0.3, -0.2, 0.1]])
    assert J.shadow_voxels_cameras(pts, cams, vps, a) == pyref.shadow_voxels_cameras(pts, cams, vps, b) and a.s == b.s


# ---- the windows of the setting --------------------------------------------------------------------------------------
def _variant_params(name):
    C_, over, _ = rc.VARIANTS[name]
    return rc.set_params(api.default_params(C_), **over)


def test_setting_zero_is_the_image_model_on_every_variant():
    assert len(rc.VARIANTS) == 24
    for name in rc.VARIANTS:
        p = _variant_params(name)
        a, b = api.ImageModel(), api.ImageModel()
        assert api.lib().gpd_hip_image_model(C.byref(p), C.byref(a)) == 0
        assert api.lib().gpd_hip_image_model_jitter(C.byref(p), 0, C.byref(b)) == 0
        for field, _ in api.ImageModel._fields_:
            assert bytes(C.string_at(C.addressof(a) + getattr(api.ImageModel, field).offset, getattr(api.ImageModel, field).size)) == \
                bytes(C.string_at(C.addressof(b) + getattr(api.ImageModel, field).offset, getattr(api.ImageModel, field).size)), (name, field)
        d0, d1 = api.image_model(p), api.image_model(p, 0)
        assert d0.keys() == d1.keys() and all(np.array_equal(d0[k], d1[k]) for k in d0), name


def test_stock_geometry_takes_the_wide_windows():
    p = api.default_params(15)
    off, on = api.image_model(p, 0), api.image_model(p, 1)
    assert off["window_class"] == 0 and (off["set_sr"], off["set_sd"]) == (43, 86)
    assert on["window_class"] == 1 and (on["set_sr"], on["set_sd"]) == (64, 128)


def test_only_the_windows_depend_on_the_setting():
    for name in rc.VARIANTS:
        p = _variant_params(name)
        off, on = api.image_model(p, 0), api.image_model(p, 1)
        for k in ("num_shadow", "stride_a", "stride_c", "true_div"):
            assert off[k] == on[k], (name, k)
        assert off["thr"].tobytes() == on["thr"].tobytes(), name
        assert on["window_class"] >= off["window_class"], name


def test_windows_follow_the_rule_with_two_more_voxels():
    """image::window_class with the jitter on: ceil(diagonal / 3 mm) + 3 + 4 voxels of window, ceil(reach / 3 mm) + 1 + 2 of
    reach, against the 46 / 42 of the default windows and the 64 / 63 of the wide ones."""
    cases = [
        (dict(volume_width=0.08, volume_depth=0.05), 0, 0),                       # 35 + 7 = 42 of 46; 37 + 3 = 40 of 42
        (dict(), 0, 1),                                                           # 42 + 7 = 49
        (dict(volume_width=0.16, volume_height=0.028), 1, 2),                     # 60 + 7 = 67 of 64
        (dict(volume_width=0.16), 1, 2),
        (dict(volume_width=0.16, volume_depth=0.10), 2, 2),
    ]
    for over, want_off, want_on in cases:
        p = api.default_params(15)
        for k, v in over.items():
            setattr(p, k, v)
        diag = math.sqrt(p.volume_depth ** 2 + p.volume_width ** 2 + 4.0 * p.volume_height ** 2)
        rx = max(p.hand_depth - p.init_bite, p.volume_depth)
        ry = 0.5 * (p.hand_outer_diameter - p.finger_width) + 0.5 * p.volume_width
        reach = math.sqrt(rx * rx + ry * ry + p.volume_height ** 2)
        for jit, want in ((0, want_off), (1, want_on)):
            win = math.ceil(diag / 0.003) + 3 + 4 * jit
            rch = math.ceil(reach / 0.003) + 1 + 2 * jit
            cls = 2 if (win > 64 or rch > 63) else (1 if (win > 46 or rch > 42) else 0)
            m = api.image_model(p, jit)
            assert cls == want == m["window_class"], (over, jit, win, rch, m["window_class"])
            if cls == 2:
                assert (m["set_sr"], m["set_sd"]) == (rch + 2, 2 * (rch + 2))


def test_model_refuses_another_setting():
    p, m = api.default_params(15), api.ImageModel()
    for bad in (2, -1):
        assert api.lib().gpd_hip_image_model_jitter(C.byref(p), bad, C.byref(m)) == GPD_ERR_INVALID
    assert api.lib().gpd_hip_image_model_jitter(None, 1, C.byref(m)) == GPD_ERR_INVALID
    assert api.lib().gpd_hip_image_model_jitter(C.byref(p), 1, None) == GPD_ERR_INVALID
