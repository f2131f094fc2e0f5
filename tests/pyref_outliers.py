"""Independent numpy restatement of Cloud::removeStatisticalOutliers (DESIGN §7 "removeStatisticalOutliers"): PCL 1.9's
StatisticalOutlierRemoval::applyFilterIndices with setMeanK / setStddevMulThresh, negative = false, on finite coordinates.
Shares no code with the host model (gpd_amd/csrc/outlier_model.h): the neighbours come from a brute-force float32 d2 matrix
(every pair, no grid, no tree), every step carries its np.float32 / np.float64 type explicitly.  For clouds of up to ~4000 points.
"""
import numpy as np

F32 = np.float32
F64 = np.float64


def sorted_d2(xyz, ranks):
    """the `ranks` smallest float32 d2 of every point to the cloud (itself included), ascending -> f32 [n, ranks].
    FLANN L2_Simple<float>: ((0 + dx*dx) + dy*dy) + dz*dz with dx = q.x - p.x, every operation rounded to float32."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    n = len(xyz)
    assert 1 <= ranks <= n
    out = np.empty((n, ranks), F32)
    for a in range(0, n, 256):
        q = xyz[a:a + 256]
        d2 = np.zeros((len(q), n), F32)
        for axis in range(3):
            d = q[:, axis][:, None] - xyz[:, axis][None, :]
            assert d.dtype == F32
            d2 = d2 + d * d
        assert d2.dtype == F32
        out[a:a + 256] = np.sort(d2, axis=1)[:, :ranks]  # equal d2 are equal addends: no tie order enters
    return out


def mean_distances(d2_sorted, mean_k):
    """item 2: ranks 1 .. mean_k in order, float32 sqrt widened, added to a float64 sum; then (float)(sum / mean_k)"""
    n = len(d2_sorted)
    assert d2_sorted.shape[1] >= mean_k + 1
    dist_sum = np.zeros(n, F64)
    for r in range(1, mean_k + 1):
        root = np.sqrt(d2_sorted[:, r])  # float32 in, float32 out: correctly rounded
        assert root.dtype == F32
        dist_sum = dist_sum + root.astype(F64)
    return (dist_sum / F64(mean_k)).astype(F32)


def statistics(dist, mult):
    """items 3-4 -> (mean, stddev, threshold) as float64; the sums run over i = 0 .. n-1 one add at a time"""
    dist = np.asarray(dist, F32)
    n = len(dist)
    sq = dist * dist  # a float32 product, rounded ...
    assert sq.dtype == F32
    wide, sq_wide = dist.astype(F64), sq.astype(F64)  # ... then widened
    total, sq_total = F64(0.0), F64(0.0)
    for i in range(n):
        total = total + wide[i]
        sq_total = sq_total + sq_wide[i]
    with np.errstate(invalid="ignore"):
        mean = total / F64(n)
        variance = (sq_total - total * total / F64(n)) / (F64(n) - F64(1.0))
        stddev = np.sqrt(variance)  # NaN for a variance that rounding made negative
        threshold = mean + F64(mult) * stddev
    return F64(mean), F64(stddev), F64(threshold), F64(variance)


def remove_statistical_outliers(xyz, mean_k, mult, d2_sorted=None):
    """-> (kept i32 ascending, stats f64 [3], dist f32 [n], variance).  Inside the domain only (1 <= mean_k, n >= mean_k + 1)."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    if d2_sorted is None:
        d2_sorted = sorted_d2(xyz, mean_k + 1)
    dist = mean_distances(d2_sorted, mean_k)
    mean, stddev, threshold, variance = statistics(dist, mult)
    with np.errstate(invalid="ignore"):
        removed = dist.astype(F64) > threshold  # False everywhere for a NaN threshold
    kept = np.flatnonzero(~removed).astype(np.int32)
    return kept, np.array([mean, stddev, threshold], F64), dist, variance
