"""Independent numpy restatement of Cloud::refineNormals (DESIGN §7 "refineNormals"): the k nearest neighbours of every point
(FLANN's float d2, ascending by (d2, index), the point itself included, k clamped to the cloud's size) and
pcl::NormalRefinement's Jacobi passes with the sequential stop rule.  Shares no code with the host model
(gpd_amd/csrc/refine_model.h): the candidates come from scipy's cKDTree, the sums are elementwise float32 array operations.
"""
import numpy as np
from scipy.spatial import cKDTree

F32 = np.float32
FLT_EPSILON = np.finfo(np.float32).eps


def flann_d2(q, p):
    """L2_Simple<float>: ((0 + dx*dx) + dy*dy) + dz*dz in float32, dx = q.x - p.x (rows of q and p)"""
    q = q.astype(F32)
    p = p.astype(F32)
    d2 = np.zeros(len(q), F32)
    for a in range(3):
        d = q[:, a] - p[:, a]
        d2 = d2 + d * d
    return d2


def knn(xyz, k):
    """-> i32 [n, min(k, n)].  cKDTree (float64) gives each point's k-th exact distance D.  A point among the first k by float
    key has float d2 <= the largest float d2 of the exact k nearest <= D^2 (1 + d), so its exact distance is at most
    D sqrt((1 + d) / (1 - d)) with d the relative error of three float32 roundings per term and two sums (< 1e-6): every point
    within D (1 + 1e-5) + 1e-15 is gathered, the float32 d2 recomputed, and the candidates sorted by (query, d2, index)."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    n = len(xyz)
    kk = min(int(k), n)
    x64 = xyz.astype(np.float64)
    tree = cKDTree(x64)
    dk, _ = tree.query(x64, k=kk)
    dk = np.asarray(dk, np.float64).reshape(n, -1)[:, -1]
    cands = tree.query_ball_point(x64, dk * (1.0 + 1e-5) + 1e-15)
    cnt = np.fromiter((len(c) for c in cands), np.int64, count=n)
    assert (cnt >= kk).all()
    qi = np.repeat(np.arange(n), cnt)
    pi = np.fromiter((i for c in cands for i in c), np.int64, count=int(cnt.sum()))
    d2 = flann_d2(xyz[qi], xyz[pi])
    order = np.lexsort((pi, d2.view(np.uint32), qi))  # last key primary: query, then d2 (>= 0: orders as its bits), then index
    start = np.concatenate(([0], np.cumsum(cnt)[:-1]))
    take = (start[:, None] + np.arange(kk)[None, :]).reshape(-1)
    return pi[order][take].reshape(n, kk).astype(np.int32)


def refine(normals, lists, max_iterations=15, convergence_threshold=1e-5):
    """NormalRefinement on float32 normals [n,3] with neighbour lists [n,k] -> (normals, passes run, means f32, non-finite count)"""
    out = np.ascontiguousarray(normals, F32).reshape(-1, 3).copy()
    n, k = lists.shape
    thr = F32(convergence_threshold)
    ddots = []
    nan3 = np.full(3, np.nan, F32)
    for _ in range(int(max_iterations)):
        s = np.zeros((n, 3), F32)
        for r in range(k):  # list order: one float32 add per rank, elementwise over the points
            v = out[lists[:, r]]
            ok = np.isfinite(v).all(axis=1)
            s = np.where(ok[:, None], s + F32(1.0) * v, s)
        norm = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        good = np.isfinite(norm) & (norm > FLT_EPSILON)
        with np.errstate(invalid="ignore", divide="ignore"):
            tmp = np.where(good[:, None], s / np.where(good, norm, F32(1))[:, None], nan3[None, :]).astype(F32)
            dot = (tmp[:, 0] * out[:, 0] + tmp[:, 1] * out[:, 1]) + tmp[:, 2] * out[:, 2]
        valid = np.isfinite(tmp).all(axis=1) & np.isfinite(dot)
        ddot = np.cumsum(dot[valid], dtype=F32)[-1] if valid.any() else F32(0)  # sequential in ascending index (never np.sum)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = F32(ddot) / F32(int(valid.sum()))
        out = tmp
        ddots.append(mean)
        if thr > 0 and F32(1.0) - mean < thr:
            break
    return out, len(ddots), np.array(ddots, F32), int((~np.isfinite(out).all(axis=1)).sum())


def refine_normals(xyz, normals, k, max_iterations=15, convergence_threshold=1e-5):
    return refine(normals, knn(xyz, k), max_iterations, convergence_threshold)
