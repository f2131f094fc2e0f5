"""An independent restatement of Cloud::sampleAbovePlane's fit (PCL 1.9's SACSegmentation, SACMODEL_PLANE,
SAC_RANSAC, optimized coefficients, then ExtractIndices(negative)) in numpy float32 scalars, plus the seeded scenes the
tests run it on.

The random stream is numpy's own MT19937 with the legacy (boost / std) seeding; atan2f, cosf and sinf come from glibc
through ctypes.  Vectorised where the definition is elementwise (the distance test), sequential where it is a chain (the
refinement's nine float sums: np.add.accumulate adds in order)."""
import ctypes as C
import sys

import numpy as np

F = np.float32
_LIBM = C.CDLL("libm.so.6")
for _name, _n in (("atan2f", 2), ("cosf", 1), ("sinf", 1)):
    getattr(_LIBM, _name).restype = C.c_float
    getattr(_LIBM, _name).argtypes = [C.c_float] * _n


def atan2f(y, x):
    return F(_LIBM.atan2f(float(y), float(x)))


def cosf(x):
    return F(_LIBM.cosf(float(x)))


def sinf(x):
    return F(_LIBM.sinf(float(x)))


class Rnd:
    """boost::uniform_int<>(0, INT_MAX) on boost::mt19937(seed): the engine's 32-bit output shifted right by one."""

    def __init__(self, seed=12345):
        self.bg = np.random.MT19937()
        self.bg._legacy_seeding(seed)

    def raw(self):
        return int(self.bg.random_raw())

    def __call__(self):
        return self.raw() >> 1


def sample_good(p0, p1, p2):
    with np.errstate(all="ignore"):
        d = (p1 - p0) / (p2 - p0)
    return bool(d[0] != d[1] or d[2] != d[1])


def plane_from3(p0, p1, p2):
    u = p1 - p0
    v = p2 - p0
    n = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], F)
    z = (n[0] * n[0] + n[2] * n[2]) + (n[1] * n[1] + F(0))
    if z > F(0):
        n = n / np.sqrt(z)
    d = -((n[0] * p0[0] + n[2] * p0[2]) + (n[1] * p0[1] + F(0) * F(1)))
    return np.array([n[0], n[1], n[2], d], F)


def inliers(c, xyz, threshold):
    """(double)|(a x + c z) + (b y + d)| < threshold, the distance in float32."""
    dist = np.abs((c[0] * xyz[:, 0] + c[2] * xyz[:, 2]) + (c[1] * xyz[:, 1] + c[3] * F(1)))
    return dist.astype(np.float64) < threshold


def roots2(b, c):
    d = F(float(b * b) - 4.0 * float(c))
    if d < F(0):
        d = F(0)
    sd = np.sqrt(d)
    return [F(0), F(0.5) * (b - sd), F(0.5) * (b + sd)]


def roots3(m):
    m00, m01, m02, m11, m12, m22 = m[0, 0], m[0, 1], m[0, 2], m[1, 1], m[1, 2], m[2, 2]
    two = F(2)
    c0 = m00 * m11 * m22 + two * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01
    c1 = m00 * m11 - m01 * m01 + m00 * m22 - m02 * m02 + m11 * m22 - m12 * m12
    c2 = m00 + m11 + m22
    if abs(c0) < np.finfo(F).eps:
        return roots2(c2, c1)
    inv3 = F(1.0 / 3.0)
    sqrt3 = np.sqrt(F(3))
    c2_3 = c2 * inv3
    a_3 = (c1 - c2 * c2_3) * inv3
    if a_3 > F(0):
        a_3 = F(0)
    half_b = F(0.5) * (c0 + c2_3 * (two * c2_3 * c2_3 - c1))
    q = half_b * half_b + a_3 * a_3 * a_3
    if q > F(0):
        q = F(0)
    rho = np.sqrt(-a_3)
    theta = atan2f(np.sqrt(-q), half_b) * inv3
    ct, st = cosf(theta), sinf(theta)
    r = [c2_3 + two * rho * ct, c2_3 - rho * (ct + sqrt3 * st), c2_3 - rho * (ct - sqrt3 * st)]
    if r[0] >= r[1]:
        r[0], r[1] = r[1], r[0]
    if r[1] >= r[2]:
        r[1], r[2] = r[2], r[1]
        if r[0] >= r[1]:
            r[0], r[1] = r[1], r[0]
    if r[0] <= F(0):
        return roots2(c2, c1)
    return r


def smallest_eigenvector(cov):
    scale = F(np.abs(cov).max())
    if scale <= np.finfo(F).tiny:
        scale = F(1)
    s = (cov / scale).astype(F)
    r0 = roots3(s)[0]
    for k in range(3):
        s[k, k] = s[k, k] - r0

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)

    vs = [cross(s[0], s[1]), cross(s[0], s[2]), cross(s[1], s[2])]
    ln = [v[0] * v[0] + (v[1] * v[1] + v[2] * v[2]) for v in vs]
    if ln[0] >= ln[1] and ln[0] >= ln[2]:
        k = 0
    elif ln[1] >= ln[0] and ln[1] >= ln[2]:
        k = 1
    else:
        k = 2
    return vs[k] / np.sqrt(ln[k])


def refine(pts):
    """computeMeanAndCovarianceMatrix (nine sequential float sums) + eigen33 -> the plane through the centroid."""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    terms = [x * x, x * y, x * z, y * y, y * z, z * z, x, y, z]
    accu = np.array([np.add.accumulate(t, dtype=F)[-1] for t in terms], F) / F(len(pts))
    cov = np.zeros((3, 3), F)
    cov[0, 0] = accu[0] - accu[6] * accu[6]
    cov[0, 1] = accu[1] - accu[6] * accu[7]
    cov[0, 2] = accu[2] - accu[6] * accu[8]
    cov[1, 1] = accu[3] - accu[7] * accu[7]
    cov[1, 2] = accu[4] - accu[7] * accu[8]
    cov[2, 2] = accu[5] - accu[8] * accu[8]
    cov[1, 0], cov[2, 0], cov[2, 1] = cov[0, 1], cov[0, 2], cov[1, 2]
    e = smallest_eigenvector(cov)
    d = -((e[0] * accu[6] + e[2] * accu[8]) + (e[1] * accu[7] + F(0) * F(1)))
    return np.array([e[0], e[1], e[2], d], F)


def fit(xyz, threshold=0.01, max_iterations=50, probability=0.99, optimize=True):
    """-> (indices off the plane, coefficients f32 [4], inliers of the final plane, iterations)."""
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    n = len(xyz)
    rnd = Rnd(12345)
    sh = list(range(n))
    best, it, k = 0, 0, sys.float_info.max
    model = None
    eps = sys.float_info.epsilon
    while it < k:
        sample = None
        if n >= 3:
            for _ in range(1000):
                for i in range(3):
                    j = i + rnd() % (n - i)
                    sh[i], sh[j] = sh[j], sh[i]
                if sample_good(xyz[sh[0]], xyz[sh[1]], xyz[sh[2]]):
                    sample = sh[:3]
                    break
        if sample is None:
            break
        c = plane_from3(xyz[sample[0]], xyz[sample[1]], xyz[sample[2]])
        count = int(inliers(c, xyz, threshold).sum())
        if count > best:
            best, model = count, c
            w = count * (1.0 / n)
            p = min(1.0 - eps, max(eps, 1.0 - w ** 3.0))
            k = np.log(1.0 - probability) / np.log(p) if probability != 1.0 else float("inf")
        it += 1
        if it > max_iterations:
            break
    if model is None:
        return np.zeros(0, np.int32), np.zeros(4, F), 0, it
    if optimize and best > 3:
        model = refine(xyz[inliers(model, xyz, threshold)])
    on = inliers(model, xyz, threshold)
    return np.flatnonzero(~on).astype(np.int32), model, int(on.sum()), it


def threshold_f32(threshold):
    """The float compare the device uses: |dist| <= this  <=>  (double)|dist| < threshold."""
    f = np.float32(threshold)
    if float(f) >= threshold:
        f = np.nextafter(f, F(-np.inf))
    return f


# ---- scenes ----------------------------------------------------------------------------------------------------------
def _rot(rng, tilt):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    ang = tilt * rng.uniform(0.2, 1.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def table_scene(rng, n_plane, n_obj, tilt=0.5, noise=0.002, lattice=None, offset=None):
    """A tilted table of n_plane points with n_obj points of boxes and spheres standing on it."""
    pl = np.c_[rng.uniform(-0.4, 0.4, (n_plane, 2)), rng.normal(0, noise, n_plane)]
    objs = []
    left = n_obj
    while left > 0:
        m = min(left, int(rng.integers(20, 200)))
        c = np.r_[rng.uniform(-0.3, 0.3, 2), 0.0]
        r = rng.uniform(0.02, 0.08)
        d = rng.normal(size=(m, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        d[:, 2] = np.abs(d[:, 2])
        objs.append(c + r * d + np.array([0, 0, r * rng.uniform(0.3, 1.2)]))
        left -= m
    pts = np.vstack([pl] + objs) if objs else pl
    pts = pts[rng.permutation(len(pts))]
    pts = pts @ _rot(rng, tilt).T + (offset if offset is not None else np.r_[0, 0, rng.uniform(0.5, 1.2)])
    if lattice:
        pts = np.round(pts / lattice) * lattice
    return pts.astype(F)


def voxelise(pts, cell):
    """One point per occupied voxel at its corner (a stand-in that leaves duplicates out) plus repeated points."""
    q = np.floor(pts / cell).astype(np.int64)
    _, first = np.unique(q, axis=0, return_index=True)
    return (q[np.sort(first)] * cell).astype(F)


def scenes(count=320, seed=2024):
    """Seeded fuzz scenes: (name, xyz f32 [n, 3], fit keyword arguments)."""
    rng = np.random.default_rng(seed)
    out = []
    for n in range(4):  # 0 / 1 / 2 / 3 points
        out.append(("tiny%d" % n, rng.uniform(-1, 1, (n, 3)).astype(F), {}))
    out.append(("three_collinear", np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], F), {}))
    # a forced zero-normal draw: every point is (0,0,0) or (1,1,0) or (1,0,1)... with duplicates: p2 == p0 and one
    # component of p1 - p0 zero passes the good-sample test with a zero cross product
    dup = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 2], [0, 0, 0], [1, 0, 2], [0, 0, 0], [3, 0, 5]], F)
    out.append(("zero_normal", dup, {}))
    out.append(("zero_normal_wide", np.repeat(dup, 7, axis=0)[rng.permutation(49)], {}))
    out.append(("plane_only", table_scene(rng, 600, 0, noise=0.0005), {}))
    out.append(("line", np.c_[np.linspace(0, 1, 50), np.linspace(0, 2, 50), np.linspace(0, 3, 50)].astype(F), {}))
    variants = [{}, {"threshold": 0.0}, {"threshold": 0.005}, {"threshold": 0.02}, {"max_iterations": 0}, {"max_iterations": 3},
                {"max_iterations": 120}, {"probability": 0.5}, {"probability": 0.999}, {"optimize": False}, {"threshold": 0.0101}]
    while len(out) < count:
        i = len(out)
        kind = i % 4
        n_plane = int(rng.integers(50, 1500))
        n_obj = int(rng.integers(0, 800))
        if kind == 0:
            xyz = table_scene(rng, n_plane, n_obj)
        elif kind == 1:
            xyz = table_scene(rng, n_plane, n_obj, lattice=0.003)
        elif kind == 2:
            xyz = voxelise(table_scene(rng, n_plane, n_obj), 0.005)
            xyz = np.vstack([xyz, xyz[rng.integers(0, len(xyz), len(xyz) // 5)]])  # duplicate coordinates
        else:
            xyz = table_scene(rng, n_plane, n_obj, tilt=1.5, noise=0.006)
        out.append(("scene%03d_k%d" % (i, kind), xyz, dict(variants[i % len(variants)])))
    return out
