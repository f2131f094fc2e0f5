"""ctypes access to the flat entry points of the host mirror (gpd_amd/host/libgpd_host.so).

The C++ classes (GraspDetector, Clustering, ...) are the product surface; this module only exposes
the `extern "C"` helpers for Python callers and tests.  No fallback: a missing library raises.
"""
import ctypes as C
import os

import numpy as np

from .api import HAND_DTYPE, _ptr

_LIB = None

_P, _I, _D = C.c_void_p, C.c_int, C.c_double
_IP = C.POINTER(C.c_int)
# every entry of gpd_amd/host/src/flat_entries.cpp: its argument types (all return int)
_ARGTYPES = {
    "gpd_host_find_clusters": [_P, _P, _I, _I, _I, _P, _P, _P],
    "gpd_host_sample_above_plane": [_P, _I, _D, _I, _D, _I, _P, _P, _IP, _IP],
    "gpd_host_refine_normals": [_P, _P, _I, _I, _I, C.c_float, _P, _P, _IP],
    "gpd_host_remove_statistical_outliers": [_P, _I, _I, _D, _P, _P, _P],
    "gpd_host_cloud_remove_statistical_outliers": [_P, _P, _P, _I, _I, _P, _I, _I, _D, _P, _P, _P, _P, _IP],
    "gpd_host_subsample_indices": [_I, _P, _I, _I, C.c_uint, _P],
    "gpd_host_knn": [_P, _I, _I, _P],
    "gpd_host_detector_refine_normals": [_P, _P, _I, _I, _P],
    "gpd_host_detector_remove_statistical_outliers": [_P, _P, _I, _P, _I, _I, _D, _P, _P, _P, _IP],
    "gpd_host_load_pcd": [C.c_char_p, _P, _P, _I, _IP],
    "gpd_host_load_normals_csv": [C.c_char_p, C.c_char_p, _P, _I],
    "gpd_host_generate_data": [C.c_char_p, _P, _IP, _IP],
}


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "libgpd_host.so")
        if not os.path.exists(path):
            raise OSError("libgpd_host.so is not built (run `make -C gpd_amd/host` or __graft_entry__.build())")
        L = C.CDLL(path)
        for name, argtypes in _ARGTYPES.items():
            getattr(L, name).argtypes = argtypes
            getattr(L, name).restype = C.c_int
        _LIB = L
    return _LIB


def find_clusters(hands, scores, min_inliers=1, remove_inliers=False):
    """Clustering::findClusters (clustering.cpp:5-105) on POD records -> (records, scores f64, seed index)."""
    hands = np.ascontiguousarray(hands, HAND_DTYPE).reshape(-1)
    scores = np.ascontiguousarray(scores, np.float64)
    assert len(scores) == len(hands)
    n = len(hands)
    out = np.zeros(max(n, 1), HAND_DTYPE)
    osc = np.zeros(max(n, 1), np.float64)
    src = np.zeros(max(n, 1), np.int32)
    k = lib().gpd_host_find_clusters(_ptr(hands), _ptr(scores), n, int(min_inliers), int(bool(remove_inliers)), _ptr(out), _ptr(osc), _ptr(src))
    return out[:k].copy(), osc[:k].copy(), src[:k].copy()


def sample_above_plane(xyz, threshold=0.01, max_iterations=50, probability=0.99, optimize=True):
    """util::Cloud::sampleAbovePlane's fit on one core (the host model) ->
    (indices off the plane i32 ascending — empty: the fit failed —, plane coefficients f32 [4], inliers, iterations)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    above = np.zeros(max(n, 1), np.int32)
    coeffs = np.zeros(4, np.float32)
    inl, its = C.c_int(0), C.c_int(0)
    k = lib().gpd_host_sample_above_plane(_ptr(xyz), n, float(threshold), int(max_iterations), float(probability), int(bool(optimize)),
                                          _ptr(above), _ptr(coeffs), C.byref(inl), C.byref(its))
    return above[:k].copy(), coeffs, int(inl.value), int(its.value)


def refine_normals(xyz, normals, k, max_iterations=15, convergence_threshold=1e-5):
    """util::Cloud::refineNormals on one core (the host model) ->
    (normals f32 [n,3] (NaN: a singularity), passes run, the stop rule's mean dot product of every pass f32, non-finite normals)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    n = len(xyz)
    out = np.zeros((max(n, 1), 3), np.float32)
    ddots = np.zeros(max(int(max_iterations), 1), np.float32)
    nan = C.c_int(0)
    its = lib().gpd_host_refine_normals(_ptr(xyz), _ptr(normals), n, int(k), int(max_iterations), float(convergence_threshold), _ptr(out),
                                        _ptr(ddots), C.byref(nan))
    return out[:n].copy(), int(its), ddots[:its].copy(), int(nan.value)


def remove_statistical_outliers(xyz, mean_k=50, stddev_mult=1.0):
    """util::Cloud::removeStatisticalOutliers' filter on one core (the host model) ->
    (kept input indices i32 ascending, stats f64 [3]: mean, stddev, threshold, mean neighbour distance of every point f32 [n]).
    ValueError outside the domain (mean_k < 1, a non-finite multiplier, fewer than mean_k + 1 points), OverflowError beyond the
    capacity (mean_k > 255)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    kept = np.zeros(max(n, 1), np.int32)
    stats = np.zeros(3, np.float64)
    dist = np.zeros(max(n, 1), np.float32)
    k = lib().gpd_host_remove_statistical_outliers(_ptr(xyz), n, int(mean_k), float(stddev_mult), _ptr(kept), _ptr(stats), _ptr(dist))
    if k == -2:
        raise OverflowError("remove_statistical_outliers: mean_k = %d, the capacity is 255" % mean_k)
    if k < 0:
        raise ValueError("remove_statistical_outliers: mean_k = %d, stddev_mult = %r on %d points is outside the domain" % (mean_k, stddev_mult, n))
    return kept[:k].copy(), stats, dist[:n].copy()


def cloud_remove_statistical_outliers(xyz, normals, cam_source, sample_indices, mean_k=50, stddev_mult=1.0):
    """util::Cloud::removeStatisticalOutliers (the C++ mirror's host method) on a cloud with normals (or None), camera-source rows
    [cams, n] and sample indices -> (xyz, normals or None, cam_source [cams, kept], sample indices) as the cloud holds them after."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    cam = np.ascontiguousarray(cam_source, np.int32).reshape(-1, n)
    si = np.ascontiguousarray(sample_indices, np.int32).reshape(-1)
    xo, no = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    co, so = np.zeros(cam.size, np.int32), np.zeros(max(len(si), 1), np.int32)
    ns = C.c_int(0)
    m = lib().gpd_host_cloud_remove_statistical_outliers(_ptr(xyz), _ptr(nrm), _ptr(cam), n, cam.shape[0], _ptr(si), len(si), int(mean_k),
                                                         float(stddev_mult), _ptr(xo), _ptr(no), _ptr(co), _ptr(so), C.byref(ns))
    if m < 0:
        raise ValueError("Cloud::removeStatisticalOutliers refused the arguments")
    return xo[:m].copy(), (None if nrm is None else no[:m].copy()), co[: cam.shape[0] * m].reshape(cam.shape[0], m).copy(), so[: ns.value].copy()


def subsample_indices(num_points, num_samples, seed=0, sample_indices=None):
    """util::Cloud::subsample on a cloud of num_points points that carries `sample_indices` (None: none) ->
    the sample indices it carries afterwards, i32."""
    lst = np.zeros(0, np.int32) if sample_indices is None else np.ascontiguousarray(sample_indices, np.int32).reshape(-1)
    out = np.zeros(max(len(lst), int(num_samples), 1), np.int32)
    k = lib().gpd_host_subsample_indices(int(num_points), _ptr(lst), len(lst), int(num_samples), int(seed) & 0xFFFFFFFF, _ptr(out))
    return out[:k].copy()


def knn(xyz, k):
    """the host model's k-nearest-neighbour lists -> i32 [n, min(k, n)], ascending by (float d2, index)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    kk = min(int(k), n)
    out = np.zeros((max(n, 1), max(kk, 1)), np.int32)
    lib().gpd_host_knn(_ptr(xyz), n, int(k), _ptr(out))
    return out[:n, :kk].copy()


def detector_refine_normals(xyz, normals, k):
    """GraspDetector::refineNormals (the device path through the C++ mirror) on a one-camera cloud -> normals f32 [n,3]."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    out = np.zeros_like(xyz)
    if lib().gpd_host_detector_refine_normals(_ptr(xyz), _ptr(normals), len(xyz), int(k), _ptr(out)) != 0:
        raise RuntimeError("GraspDetector::refineNormals failed")
    return out


def detector_remove_statistical_outliers(xyz, normals, sample_indices, mean_k=50, stddev_mult=1.0):
    """GraspDetector::removeStatisticalOutliers (the device path through the C++ mirror) on a one-camera cloud ->
    (xyz f32 [m,3], normals f32 [m,3], sample indices i32) as the cloud holds them afterwards."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    si = np.ascontiguousarray(sample_indices, np.int32).reshape(-1)
    xo, no, so = np.zeros_like(xyz), np.zeros_like(xyz), np.zeros(max(len(si), 1), np.int32)
    ns = C.c_int(0)
    m = lib().gpd_host_detector_remove_statistical_outliers(_ptr(xyz), _ptr(normals), len(xyz), _ptr(si), len(si), int(mean_k), float(stddev_mult),
                                                            _ptr(xo), _ptr(no), _ptr(so), C.byref(ns))
    if m < 0:
        raise RuntimeError("GraspDetector::removeStatisticalOutliers failed")
    return xo[:m].copy(), no[:m].copy(), so[: ns.value].copy()


def load_pcd(path, cap=1 << 22):
    """util::Cloud(filename): ASCII or uncompressed binary PCD -> (xyz f32 [n,3], normals f32 [n,3] or None)."""
    xyz = np.zeros((cap, 3), np.float32)
    nrm = np.zeros((cap, 3), np.float32)
    has = C.c_int(0)
    n = lib().gpd_host_load_pcd(str(path).encode(), _ptr(xyz), _ptr(nrm), cap, C.byref(has))
    n = min(n, cap)
    return xyz[:n].copy(), (nrm[:n].copy() if has.value else None)


def generate_data(config, trainer):
    """DataGenerator::generateData(sink) of the config file into the resident sets of `trainer` (api.Trainer): every view is one
    gpd_hip_train_append_view, every object's ranges are shuffled on the device, no .npy file is written -> (n_train, n_test)
    generated."""
    n_train, n_test = C.c_int(0), C.c_int(0)
    if lib().gpd_host_generate_data(str(config).encode(), trainer._h, C.byref(n_train), C.byref(n_test)) != 0:
        raise RuntimeError("generate_data into the trainer failed (the C++ side printed why)")
    return int(n_train.value), int(n_test.value)
