"""Clouds that send points down every route of estimate_normals (gpd_amd/csrc/normals.hip) at its boundary, and numpy
restatements — independent of the oracle — of what decides the route: the neighbour counts, the queue and its sort space,
the arena demand, the centroid certificate, the uniform grid.  tests/test_normals_routes_host.py checks these helpers against
the oracle's own neighbour lists on the CPU; tests/test_gpu_normals_routes.py holds the device to them.

The rules restated (each from the kernel's text, none from its output):
  count     FLANN L2_Simple<float>: d2 accumulated in float32 over x, y, z, a neighbour iff d2 < float32(radius * radius), self included
  route     count <= 256 / 512 / 1024: a wave sorts 4 / 8 / 16 keys per lane; beyond 1024 the point is queued and a workgroup sorts
            m = 2^ceil(log2 count) keys, in LDS while m <= 8192, else in m slots of the arena
  arena     every queued point draws m slots, per tile of 65536 cell-order positions; a fresh context holds 2^20; a run that asks
            for more grows the arena to demand + demand / 8 and is repeated (attempts = 2)
  centroid  the order-free fp64 sum is certified per axis by centre_exact(emin, emax, count); the exponents come from the entries
            when the query is within 2 * rad of a coordinate plane on some axis (rad = sqrtf(r2) * 1.0001f), else from
            |q| + rad and |q| - rad (one binade of slack); a point that is not queued and fails on some axis walks its chains
"""
import numpy as np

RADIUS = 0.03
NL_CAP = 1024        # neighbours a wave sorts in registers
BIG_LDS = 8192       # keys the workgroup kernel sorts in LDS
TILE = 65536         # cell-order positions per pass
ARENA_FRESH = 1 << 20  # slots of a fresh context's arena
CAM1 = np.zeros((1, 3))


# ---------------------------------------------------------------------------------------------------------------- clouds
def oblate_blob(rng, n, centre, radius=0.012, squash=0.3):
    """n points uniform in a ball of `radius`, z scaled by `squash`: every pair within 2 * radius, the normal along z"""
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    p = v * (radius * rng.uniform(size=n) ** (1.0 / 3.0))[:, None]
    p[:, 2] *= squash
    return (np.asarray(centre, np.float64) + p).astype(np.float32)


def boundary_cloud(sizes, seed):
    """one oblate blob of exactly B points per entry of `sizes`, 0.3 m apart, each with ONE satellite 0.03 m from its centre: the
    blob's points have B or B + 1 neighbours.  -> dict(xyz, cam, vp, blobs=[(first index, B, satellite index)])"""
    rng = np.random.RandomState(seed)
    parts, blobs, at = [], [], 0
    for k, B in enumerate(sizes):
        c = np.array([0.3 + 0.3 * k, 0.3, 0.5])
        parts.append(oblate_blob(rng, B, c))
        parts.append((c + np.array([0.0, 0.03, 0.0])).astype(np.float32)[None])
        blobs.append((at, B, at + B))
        at += B + 1
    xyz = np.ascontiguousarray(np.concatenate(parts))
    return dict(xyz=xyz, cam=np.ones((1, len(xyz)), np.int32), vp=CAM1.copy(), blobs=blobs)


def small_blobs():
    """256, 512 and 1024: the three register sorts and the queue at their boundaries, in one cloud of 1795 points"""
    return boundary_cloud((256, 512, 1024), 11)


def degenerate_cloud():
    """a lone point, a pair, three collinear points, five identical points, a 5 x 5 coplanar 3 mm lattice and an ordinary blob
    that no camera of a two-camera rig sees.  -> dict(xyz, cam, vp, parts={name: index range})"""
    rng = np.random.RandomState(12)
    base = lambda k: np.array([0.25 + 0.25 * k, 0.25, 0.5])  # (multiples of 1 / 4: the small offsets below add exactly)
    step = np.array([2.0 ** -8, 2.0 ** -7, 0.0])
    gi, gj = np.meshgrid(np.arange(5), np.arange(5), indexing="ij")
    clusters = [
        ("lone", base(0)[None]),
        ("pair", base(1) + np.array([[0, 0, 0], [0.004, 0.003, 0.0]])),
        ("collinear", base(2) + np.arange(3)[:, None] * step),
        ("identical", np.tile(base(3) + np.array([0.001, 0.002, 0.003]), (5, 1))),
        ("lattice", base(4) + np.stack([gi.ravel() * 0.003, gj.ravel() * 0.003, np.zeros(25)], 1)),
        ("unseen", oblate_blob(rng, 300, base(5))),
    ]
    seen = dict(lone=(1, 0), pair=(0, 1), collinear=(1, 1), identical=(1, 0), lattice=(0, 1), unseen=(0, 0))
    xyz, cam, parts, at = [], [], {}, 0
    for name, p in clusters:
        p = np.asarray(p, np.float64).astype(np.float32)
        xyz.append(p)
        cam.append(np.tile(np.array(seen[name], np.int32)[:, None], (1, len(p))))
        parts[name] = range(at, at + len(p))
        at += len(p)
    return dict(xyz=np.ascontiguousarray(np.concatenate(xyz)), cam=np.ascontiguousarray(np.concatenate(cam, 1)),
                vp=np.array([[0.0, 0.0, 0.0], [0.3, -0.2, 0.1]]), parts=parts)


def tiled_cloud():
    """a jittered 4 mm sheet of 66 000 points (every neighbourhood below 256) and a blob of 1100 at the largest x: x is the
    slowest axis of the cell order, so the blob's positions lie behind the first tile of 65536"""
    rng = np.random.RandomState(13)
    gi, gj = np.meshgrid(np.arange(660), np.arange(100), indexing="ij")
    sheet = np.stack([0.1 + gi.ravel() * 0.004, 0.1 + gj.ravel() * 0.004, np.full(gi.size, 0.5)], 1)
    sheet += rng.uniform(-0.0012, 0.0012, sheet.shape) * np.array([1.0, 1.0, 0.25])
    blob = oblate_blob(rng, 1100, [sheet[:, 0].max() + 0.25, 0.3, 0.5])
    xyz = np.ascontiguousarray(np.concatenate([sheet.astype(np.float32), blob]))
    return dict(xyz=xyz, cam=np.ones((1, len(xyz)), np.int32), vp=CAM1.copy(), blob=range(len(sheet), len(xyz)))


def strip_cloud():
    """1500 points in a strip along y (0.5 .. 0.75 m), 4 mm thick across the plane x = 0, and ONE point with x = 1e-12 at the far
    end: its neighbours' x sums span 2^-40 .. 2^-9 and are refused by the certificate; the rest of the strip (every point is within
    2 * rad of the plane, so every neighbourhood tracks its entries) is certified"""
    rng = np.random.RandomState(14)
    p = np.stack([rng.uniform(-0.002, 0.002, 1500), rng.uniform(0.5, 0.75, 1500), 0.5 + rng.uniform(-0.0005, 0.0005, 1500)], 1).astype(np.float32)
    tiny = np.array([[1e-12, 0.75, 0.5]], np.float32)
    xyz = np.ascontiguousarray(np.concatenate([p, tiny]))
    return dict(xyz=xyz, cam=np.ones((1, len(xyz)), np.int32), vp=CAM1.copy(), tiny=len(xyz) - 1)


def with_far_pair(xyz, gap):
    """the cloud plus two points `gap` metres apart along x, around its middle: the grid's extent decides its cell"""
    mid = (xyz.min(0).astype(np.float64) + xyz.max(0)) / 2
    far = np.stack([mid - [gap / 2, 0, 0], mid + [gap / 2, 0, 0]]).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([xyz, far]))


def flat_cloud():
    """2000 points of a jittered sheet with every z equal: the grid has ONE layer"""
    rng = np.random.RandomState(15)
    p = np.stack([rng.uniform(0.1, 0.4, 2000), rng.uniform(0.1, 0.3, 2000), np.full(2000, 0.5)], 1)
    return np.ascontiguousarray(p.astype(np.float32))


# ---------------------------------------------------------------------------------------- neighbourhoods by brute force
def neighbourhoods(xyz, radius, chunk=256):
    """yields (rows, candidates, mask): for `rows` (indices into xyz) the boolean matrix of neighbours among `candidates`.  Brute
    force in float32, as the kernel documents FLANN; the only shortcut is sound: points farther than the radius along x alone
    (by a margin far above float32 rounding) are not candidates."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    r2 = np.float32(radius * radius)
    order = np.argsort(xyz[:, 0], kind="stable")
    xs = xyz[order, 0].astype(np.float64)
    w = radius * 1.01 + 1e-4
    for a in range(0, len(xyz), chunk):
        rows = order[a:a + chunk]
        lo = np.searchsorted(xs, xs[a] - w, "left")
        hi = np.searchsorted(xs, xs[min(a + chunk, len(xyz)) - 1] + w, "right")
        cand = order[lo:hi]
        q, c = xyz[rows], xyz[cand]
        d = q[:, None, 0] - c[None, :, 0]
        d2 = d * d
        d = q[:, None, 1] - c[None, :, 1]
        d2 = d2 + d * d
        d = q[:, None, 2] - c[None, :, 2]
        d2 = d2 + d * d
        assert d2.dtype == np.float32
        yield rows, cand, d2 < r2


def counts(xyz, radius):
    """neighbours of every point within the radius, the point itself included -> int32 [P]"""
    out = np.zeros(len(xyz), np.int32)
    for rows, _, mask in neighbourhoods(xyz, radius):
        out[rows] = mask.sum(1)
    return out


def lists(xyz, radius):
    """the neighbour sets themselves (small clouds) -> list of sorted index arrays"""
    out = [None] * len(xyz)
    for rows, cand, mask in neighbourhoods(xyz, radius):
        for r, m in zip(rows, mask):
            out[r] = np.sort(cand[m])
    return out


# ------------------------------------------------------------------------------------------------------------ the routes
def pow2ceil(n):
    n = np.asarray(n, np.int64)
    m = np.ones_like(n)
    for _ in range(40):
        m = np.where(m < n, m * 2, m)
    return m


def tally(count, tile=None, arena_before=ARENA_FRESH):
    """what gpd_hip_last_normals_routes must report for these counts (all but the centroid chains).  tile: per point, the tile its
    cell-order position lies in (None: one tile); arena_before: the context's arena before the call, in slots."""
    count = np.asarray(count, np.int64)
    P = len(count)
    tiles = (P + TILE - 1) // TILE
    tile = np.zeros(P, np.int64) if tile is None else np.asarray(tile, np.int64)
    queued = count > NL_CAP
    m = pow2ceil(count)
    demand = max([int(m[queued & (tile == t)].sum()) for t in range(tiles)] + [0])  # the arena is the next tile's again
    grown = demand > arena_before
    return dict(points=P, tiles=tiles, queued=int(queued.sum()), queued_lds=int((queued & (m <= BIG_LDS)).sum()),
                queued_arena=int((queued & (m > BIG_LDS)).sum()), attempts=2 if grown else 1,
                arena_slots=demand + demand // 8 if grown else arena_before), demand


def register_routes(count):
    """points per register sort (keys per lane) -> {4: .., 8: .., 16: ..}"""
    count = np.asarray(count)
    return {4: int((count <= 256).sum()), 8: int(((count > 256) & (count <= 512)).sum()), 16: int(((count > 512) & (count <= NL_CAP)).sum())}


def some_wave_is_mixed(k, P):
    """k of P points have a property; a wave is 64 consecutive cell-order positions (the last one P % 64).  If every wave held only
    points with it or only points without, k would be a sum of whole waves: a multiple of 64, plus P % 64 if the last one is in."""
    return k % 64 not in (0, P % 64)


# -------------------------------------------------------------------------------------------------------------- the grid
def grid_of(xyz):
    """cloud_upload's uniform grid: 2 cm cells, doubled until no axis has more than 256 -> (lo f32 [3], cell f32, dim int [3])"""
    xyz = np.asarray(xyz, np.float32)
    lo, hi = xyz.min(0), xyz.max(0)
    cell = np.float32(0.02)
    while True:
        dim = np.floor((hi - lo) / cell).astype(np.int64) + 1
        if (dim <= 256).all() and (dim >= 1).all():
            return lo, cell, dim
        cell = np.float32(cell * np.float32(2))


def grid_coord(v, axis, grid):
    lo, cell, dim = grid
    k = np.floor((np.asarray(v, np.float32) - lo[axis]) / cell).astype(np.int64)
    return np.clip(k, 0, dim[axis] - 1)


def cell_columns(xyz, radius):
    """(x, y) cell columns normals_visit finds around every point: more than 64 send the wave through grid_visit"""
    g = grid_of(xyz)
    reach = np.float32(np.float32(radius) * np.float32(1.001) + np.float32(1e-5))
    xyz = np.asarray(xyz, np.float32)
    nx = grid_coord(xyz[:, 0] + reach, 0, g) - grid_coord(xyz[:, 0] - reach, 0, g) + 1
    ny = grid_coord(xyz[:, 1] + reach, 1, g) - grid_coord(xyz[:, 1] - reach, 1, g) + 1
    return nx * ny


def positions_before(xyz, rows):
    """a lower bound of the cell-order position of every point of `rows`: the points in grid slices of a smaller x (x is the slowest
    axis of the cell index; the order inside a slice, and inside a cell, is not stated here)"""
    g = grid_of(xyz)
    cx = grid_coord(np.asarray(xyz, np.float32)[:, 0], 0, g)
    return int((cx < cx[np.asarray(rows)].min()).sum())


# ------------------------------------------------------------------------------------------------------- the certificate
def _bexp(bits):
    e = (np.asarray(bits, np.int64) >> 23) & 0xFF
    return np.where(e == 0, 1, e)


def _bits(x):
    return np.abs(np.asarray(x, np.float32)).view(np.uint32).astype(np.int64)


def centre_exact(emin, emax, n):
    """grid_sort.h centre_exact on arrays"""
    emin, emax, n = (np.asarray(a, np.int64) for a in (emin, emax, n))
    lg = np.zeros_like(n)
    for k in range(40):
        lg += ((1 << k) < n).astype(np.int64)
    return (emax == 0) | ((emax < 255) & (lg + emax - emin <= 28))


def centroid_chains(xyz, radius):
    """normals_sort_store's rule -> (chain bool [P]: the point's centroid is NOT certified on some axis, count int32 [P]).
    Only a point that is not queued (count <= 1024) has a centroid from that kernel."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    r2 = np.float32(radius * radius)
    rad = np.float32(np.sqrt(r2) * np.float32(1.0001))
    assert rad.dtype == np.float32
    two = np.float32(np.float32(2) * rad)
    chain = np.zeros(len(xyz), bool)
    count = np.zeros(len(xyz), np.int32)
    for rows, cand, mask in neighbourhoods(xyz, radius):
        q = xyz[rows]
        n = mask.sum(1)
        count[rows] = n
        track = ~(np.abs(q) > two).all(1)
        bad = np.zeros(len(rows), bool)
        for a in range(3):
            b = _bits(xyz[cand, a])
            live = mask & (b != 0)[None, :]
            hi = np.where(live, b[None, :], 0).max(1)
            lo = np.where(live, b[None, :], 1 << 32).min(1)
            emax_t = np.where(hi > 0, _bexp(hi), 0)
            emin_t = np.where(hi > 0, _bexp(lo), 255)
            aq = np.abs(q[:, a])
            emax_u = _bexp(_bits(aq + rad))
            emin_u = _bexp(_bits(aq - rad)) - 1
            emax, emin = np.where(track, emax_t, emax_u), np.where(track, emin_t, emin_u)
            bad |= ~centre_exact(emin, emax, n)
        chain[rows] = bad
    return chain, count


# ---------------------------------------------------------------------------------------------- an independent fp64 form
def eigh_normals(xyz, radius):
    """per point: float64 centroid and covariance of its brute-force neighbours, numpy.linalg.eigh -> (unit eigenvector of the
    smallest eigenvalue f64 [P, 3], relative gap (l_mid - l_min) / l_max [P])"""
    x64 = np.asarray(xyz, np.float64)
    nrm = np.zeros((len(xyz), 3))
    gap = np.zeros(len(xyz))
    for i, nb in enumerate(lists(xyz, radius)):
        p = x64[nb]
        d = p - p.mean(0)
        w, v = np.linalg.eigh(d.T @ d)
        nrm[i] = v[:, 0]
        gap[i] = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0
    return nrm, gap
