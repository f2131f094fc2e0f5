"""The host arithmetic of the image stage, no GPU: gpd_hip_image_model (gpd_amd/csrc/image_model.h — the window class of an
image volume, the exact cell thresholds, the LCG jump of the shadow draws, the self-check of the division by a constant),
the values images_reserve / images_run hand the kernels."""
import ctypes as C
import math

import numpy as np
import pytest

from gpd_amd import api

GPD_ERR_CAPACITY = -3

# geometry -> (window class, set_sr, set_sd), from the rule of image::window_class: the candidate window holds
# ceil(diagonal / 3 mm) + 3 voxels, the set region ceil(reach / 3 mm) + 1.  The default sits on the boundary of class 0:
# 45 of 46 window voxels, 42 of 42 voxels of reach.
GEOMETRIES = [
    (dict(), (0, 43, 86)),
    (dict(volume_width=0.16, volume_height=0.028), (1, 64, 128)),
    (dict(volume_width=0.16), (1, 64, 128)),
    (dict(volume_width=0.16, volume_depth=0.10), (2, 60, 120)),
    (dict(volume_width=0.30, volume_depth=0.20, volume_height=0.10), (2, 105, 210)),
]


def _params(over):
    p = api.default_params(15)
    for k, v in over.items():
        setattr(p, k, v)
    return p


@pytest.fixture(scope="module")
def models():
    return [(_params(over), api.image_model(_params(over))) for over, _ in GEOMETRIES]


def test_window_class_of_each_geometry(models):
    for (over, want), (_, m) in zip(GEOMETRIES, models):
        assert (m["window_class"], m["set_sr"], m["set_sd"]) == want, over


def test_a_volume_of_metres_is_refused():
    p, m = _params(dict(volume_depth=2.0)), api.ImageModel()
    assert api.lib().gpd_hip_image_model(C.byref(p), C.byref(m)) == GPD_ERR_CAPACITY
    assert b"beyond the shadow region" in api.lib().gpd_hip_last_error()
    with pytest.raises(api.GpdHipError):
        api.image_model(p)
    assert api.lib().gpd_hip_image_model(None, C.byref(m)) == -1 and api.lib().gpd_hip_image_model(C.byref(p), None) == -1


def test_thresholds_are_the_first_doubles_of_their_cells(models):
    """thr[k] is the smallest double the reference's cell formula floor((x / len) / (1 / 60)) puts into cell k or beyond:
    the formula in numpy's float64 (the same IEEE divisions) says >= k at thr[k] and < k one double below."""
    cell = np.float64(1.0) / np.float64(60.0)
    k = np.arange(1, 60)
    for p, m in models[:2]:
        lens = (p.volume_depth, p.volume_width, 2.0 * p.volume_height)
        assert m["thr"].shape == (3, 61)
        for a, ln in enumerate(lens):
            thr, ln = m["thr"][a], np.float64(ln)
            assert thr[0] == 0.0 and thr[60] == np.finfo(np.float64).max
            at = np.floor((thr[1:60] / ln) / cell)
            below = np.floor((np.nextafter(thr[1:60], 0.0) / ln) / cell)
            assert np.all(at >= k), (a, float(ln), k[at < k])
            assert np.all(below < k), (a, float(ln), k[below >= k])
            assert np.all(np.diff(thr) > 0)


def test_shadow_draws_and_the_jump_over_a_workgroup(models):
    """num_shadow draws per point; a thread of shadow_set_kernel (1024 of them) moves on by 1024 * num_shadow draws with ONE
    affine map: the composition of that many single steps of HandSet::fastrand, here step by step."""
    for p, m in models:
        assert m["num_shadow"] == math.floor(max(p.volume_depth, p.volume_height / 2.0, p.volume_width) / 0.003)
        A, Cc = 1, 0
        for _ in range(1024 * m["num_shadow"]):
            A, Cc = (214013 * A) % 2 ** 32, (214013 * Cc + 2531011) % 2 ** 32
        assert (m["stride_a"], m["stride_c"]) == (A, Cc)
        s = 12345
        for _ in range(1024 * m["num_shadow"]):
            s = (214013 * s + 2531011) % 2 ** 32
        assert (m["stride_a"] * 12345 + m["stride_c"]) % 2 ** 32 == s


def test_default_extents_divide_through_the_reciprocal(models):
    assert models[0][1]["true_div"] == 0


def test_the_model_does_not_depend_on_what_was_asked_before(models):
    """the per-axis cache of image::fill_consts holds one geometry: asking for another and coming back gives the same block"""
    for (p, m) in models[:2] + models[:1]:
        again = api.image_model(p)
        assert again["thr"].tobytes() == m["thr"].tobytes()
        assert {k: v for k, v in again.items() if k != "thr"} == {k: v for k, v in m.items() if k != "thr"}
