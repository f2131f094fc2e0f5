"""Every route of estimate_normals (gpd_amd/csrc/normals.hip) at its boundary, and proof that it ran.

Each cloud of tests/normals_route_cases.py is compared with TWO references: the oracle's normals byte for byte (tobytes: a
point no camera sees gives -0.0, which array_equal cannot tell from +0.0), and the brute-force float32 neighbour counts of that
module, which the per-point counts of Context.normals_routes() (gpd_hip_last_normals_routes) must equal exactly.  From those
counts — from the inputs, never from the device — follows how many points took each route, the arena's demand, whether the run
had to be repeated and how many centroid chains were walked; the report must equal that, number for number.

  route                                              test
  register sorts <4>, <8>, <16> at 256/257, 512/513  test_small_blobs_take_every_register_sort_and_the_queue
  the queue at 1024/1025; small and queued lanes     (the same)
  one attempt below 2^20 slots of demand             (the same)
  LDS sort at 4096/4097 (the padding doubles)        test_blob_of_4096_is_sorted_in_lds_on_the_second_attempt
  LDS / arena sort at 8192/8193, the arena grows     test_blob_of_8192_is_sorted_in_lds_and_in_the_arena
  rank 0 / 1 / 2 covariance, duplicates, -0.0        test_degenerate_neighbourhoods
  a queued point in the second tile, then a small    test_queued_points_behind_the_first_tile
  cloud on the same context
  centroid certificate refused beside certified      test_centroid_certificate_refused_and_certified_in_one_strip
  more than 64 cell columns (grid_visit)             test_many_cell_columns
  cells of 0.04 / 0.16, one layer, one point; the    test_coarse_and_flat_grids
  coarse grid under search, outliers, refinement
  float64 covariance + numpy.linalg.eigh             test_independent_float64_form
"""
import numpy as np
import pytest

import normals_route_cases as K
import test_outlier_model as OM
import test_refine_normals_model as RM
from gpd_amd import api, hostlib, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(api.default_params(15))
    yield c
    c.close()


def _expected(xyz, radius, tile=None, arena_before=K.ARENA_FRESH):
    """the report the inputs demand -> (info, counts, slot demand)"""
    chain, count = K.centroid_chains(xyz, radius)
    info, demand = K.tally(count, tile, arena_before)
    info["centroid_chains"] = int((chain & (count <= K.NL_CAP)).sum())
    return info, count, demand


def _run(ctx, oracle_mod, xyz, cam, vp, radius=K.RADIUS, tile=None, arena_before=K.ARENA_FRESH):
    """upload, estimate, report; the normals against the oracle's bytes, the counts and the routes against the restatement.
    arena_before None: a context whose arena is not known (attempts and the arena size are left out)."""
    ctx.upload_cloud(xyz, np.zeros_like(xyz), cam, vp)
    got = ctx.estimate_normals(radius)
    count, info = ctx.normals_routes()
    want_info, want_count, demand = _expected(xyz, radius, tile, K.ARENA_FRESH if arena_before is None else arena_before)
    assert np.array_equal(count, want_count), np.flatnonzero(count != want_count)[:10]
    if arena_before is None:
        for k in ("attempts", "arena_slots"):
            info.pop(k), want_info.pop(k)
    assert info == want_info
    want = oracle_mod.estimate_normals(xyz, cam, vp, radius)
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[:10]
    return got, count, info, demand


@pytest.fixture(scope="module")
def small_run(oracle_mod):
    """the three small blobs on a fresh context, run once (the float64 form reads the same result)"""
    c = K.small_blobs()
    fresh = api.Context(api.default_params(15))
    try:
        got, count, info, demand = _run(fresh, oracle_mod, c["xyz"], c["cam"], c["vp"])
    finally:
        fresh.close()
    return dict(c, got=got, count=count, info=info, demand=demand)


def _both_sides(c, count):
    for first, B, sat in c["blobs"]:
        assert set(count[first:first + B].tolist()) == {B, B + 1}, B


def test_small_blobs_take_every_register_sort_and_the_queue(small_run):
    r = small_run
    _both_sides(r, r["count"])  # 256/257, 512/513, 1024/1025 all occur
    routes = K.register_routes(r["count"])
    assert min(routes.values()) > 0 and sum(routes.values()) + r["info"]["queued"] == len(r["count"])
    assert r["info"]["queued"] == r["info"]["queued_lds"] == int((r["count"] == 1025).sum()) > 0
    # the demand was put BELOW the fresh arena's 2^20 slots: one attempt, the arena as created
    assert r["demand"] == 2048 * r["info"]["queued"] < K.ARENA_FRESH
    assert r["info"]["attempts"] == 1 and r["info"]["arena_slots"] == K.ARENA_FRESH and r["info"]["tiles"] == 1
    assert r["info"]["centroid_chains"] == 0
    assert K.some_wave_is_mixed(r["info"]["queued"], len(r["count"]))  # the finish kernel's per-lane walk with both kinds of lanes


def test_blob_of_4096_is_sorted_in_lds_on_the_second_attempt(oracle_mod):
    """4096 neighbours sort as 4096 keys, 4097 as 8192: both in LDS.  The demand (24.8 M slots) is beyond a fresh arena: two attempts."""
    c = K.boundary_cloud((4096,), 20 + 4096)
    fresh = api.Context(api.default_params(15))
    try:
        got, count, info, demand = _run(fresh, oracle_mod, c["xyz"], c["cam"], c["vp"])
    finally:
        fresh.close()
    _both_sides(c, count)
    assert info["queued"] == info["queued_lds"] == len(count) and info["queued_arena"] == 0
    assert info["attempts"] == 2 and info["arena_slots"] == demand + demand // 8


def test_blob_of_8192_is_sorted_in_lds_and_in_the_arena(oracle_mod):
    """8192 neighbours sort as 8192 keys in LDS, 8193 as 16384 keys in the point's arena slice.  The cloud asks for 97 947 648 sort
    slots; the arena grows from 8 MB to 110 191 104 slots (0.88 GB) and the run is repeated: attempts == 2."""
    c = K.boundary_cloud((8192,), 20 + 8192)
    fresh = api.Context(api.default_params(15))
    try:
        got, count, info, demand = _run(fresh, oracle_mod, c["xyz"], c["cam"], c["vp"])
    finally:
        fresh.close()
    _both_sides(c, count)
    assert info["queued"] == len(count)
    assert info["queued_lds"] == int((count <= 8192).sum()) > 0 and info["queued_arena"] == int((count == 8193).sum()) > 0
    assert info["attempts"] == 2 and info["arena_slots"] == demand + demand // 8 == 110191104
    print("8192 blob: %d slots asked for, arena %d slots = %.3f GB" % (demand, info["arena_slots"], 8e-9 * info["arena_slots"]))


def test_degenerate_neighbourhoods(ctx, oracle_mod):
    """eigen3 on a zero, a rank-1 and a rank-2 matrix, five keys with equal distance bits, and a blob no camera sees"""
    c = K.degenerate_cloud()
    got, count, info, _ = _run(ctx, oracle_mod, c["xyz"], c["cam"], c["vp"], arena_before=None)
    for name, rows in c["parts"].items():
        assert (count[list(rows)] == len(rows)).all(), name
    assert info["queued"] == 0 and info["centroid_chains"] == 0
    unseen = got[list(c["parts"]["unseen"])]
    assert (unseen.view(np.uint32) == 0x80000000).all()  # (-0.0, -0.0, -0.0): never estimated, then reversed
    seen = got[: c["parts"]["unseen"][0]]
    assert np.isfinite(seen).all()
    lattice = got[list(c["parts"]["lattice"])]
    assert np.abs(np.abs(lattice[:, 2]) - 1).max() < 1e-6  # the plane's normal


def test_queued_points_behind_the_first_tile(oracle_mod):
    """67 100 points run as two tiles of cell-order positions; the 1100 queued points all lie in the second one (w0 > 0), whose
    queue, arena and lists are the first tile's again.  Their 2 252 800 slots are beyond a fresh arena: two attempts.  Then a small
    cloud on the same context: one tile, nothing queued, the grown arena kept."""
    c = K.tiled_cloud()
    assert K.positions_before(c["xyz"], c["blob"]) >= K.TILE
    tile = np.zeros(len(c["xyz"]), int)
    tile[list(c["blob"])] = 1
    fresh = api.Context(api.default_params(15))
    try:
        got, count, info, demand = _run(fresh, oracle_mod, c["xyz"], c["cam"], c["vp"], tile=tile)
        assert info["tiles"] == 2 and info["queued"] == int((count > 1024).sum()) == 1100 == info["queued_lds"]
        assert info["attempts"] == 2 and info["arena_slots"] == demand + demand // 8
        cl = synth.make_cloud(78, 2000)
        _, count2, info2, _ = _run(fresh, oracle_mod, cl["xyz"], cl["cam_source"], cl["view_points"], arena_before=info["arena_slots"])
        assert info2["tiles"] == 1 and info2["queued"] == 0 and info2["attempts"] == 1 and info2["points"] == 2000
    finally:
        fresh.close()


def test_centroid_certificate_refused_and_certified_in_one_strip(ctx, oracle_mod):
    """normals_sort_store's certificate on the `track` branch: the neighbours of a point 1e-12 m from the plane x = 0 are refused
    (NaN, their chains walked by normals_finish_kernel), the rest of the strip is certified, and some wave holds both."""
    c = K.strip_cloud()
    chain, n = K.centroid_chains(c["xyz"], K.RADIUS)
    got, count, info, _ = _run(ctx, oracle_mod, c["xyz"], c["cam"], c["vp"], arena_before=None)
    assert info["centroid_chains"] == int(chain.sum()) == int(count[c["tiny"]])
    assert 0 < info["centroid_chains"] < len(count) and info["queued"] == 0
    assert K.some_wave_is_mixed(info["centroid_chains"], len(count))


def test_many_cell_columns(ctx, oracle_mod):
    """radius 0.07: neighbourhoods of up to 64 and of more cell columns in one launch; radius 0.1: more of the latter"""
    cl = synth.make_cloud(77, 3000)
    wide = {}
    for radius in (0.07, 0.1):
        col = K.cell_columns(cl["xyz"], radius)
        wide[radius] = int((col > 64).sum())
        assert 0 < wide[radius] < len(col)
        _run(ctx, oracle_mod, cl["xyz"], cl["cam_source"], cl["view_points"], radius, arena_before=None)
    assert wide[0.07] < wide[0.1]
    print("points with more than 64 cell columns:", wide)


def test_coarse_and_flat_grids(ctx, oracle_mod):
    """an extent beyond 5.12 m doubles the grid's cell (0.04, then 0.16 at 30 m); equal z gives one layer; one point gives one cell.
    The coarse grid lies under the search, the outlier filter and the refinement as well."""
    cl = synth.make_cloud(77, 3000)
    one = np.ones((1, 1), np.int32)
    for gap, cell in ((6.0, 0.04), (30.0, 0.16)):
        xyz = K.with_far_pair(cl["xyz"], gap)
        assert K.grid_of(xyz)[1] == np.float32(cell)
        _run(ctx, oracle_mod, xyz, np.ones((1, len(xyz)), np.int32), K.CAM1, arena_before=None)
    flat = K.flat_cloud()
    assert K.grid_of(flat)[2][2] == 1
    _run(ctx, oracle_mod, flat, np.ones((1, len(flat)), np.int32), K.CAM1, arena_before=None)
    got, count, info, _ = _run(ctx, oracle_mod, cl["xyz"][:1].copy(), one, K.CAM1, arena_before=None)
    assert count.tolist() == [1] and info["points"] == 1
    # the 6 m cloud under the other searches
    xyz = K.with_far_pair(cl["xyz"], 6.0)
    nrm = np.ascontiguousarray(np.concatenate([cl["normals"], cl["normals"][:2]]))
    ctx.upload_cloud(xyz, nrm)
    rng = np.random.RandomState(5)
    sm = xyz[rng.choice(np.flatnonzero(cl["is_object"]), 16, replace=False)].astype(np.float64) + rng.uniform(-0.003, 0.003, (16, 3))
    hands = ctx.search_samples(sm)
    want = oracle_mod.search_xyz(oracle_mod.default_params(15), xyz, nrm, sm)
    assert hands.shape == want.shape and hands.tobytes() == want.tobytes() and want["valid"].any()
    dev = ctx.refine_normals(10)
    host = hostlib.refine_normals(xyz, nrm, 10)
    RM.assert_same_normals(dev[0], host[0])
    assert dev[1] == host[1] and dev[3] == host[3] and dev[2].view(np.uint32).tolist() == host[2].view(np.uint32).tolist()
    ctx.upload_cloud(xyz, nrm)
    kept = ctx.remove_statistical_outliers(50, 1.0)
    OM.assert_same(kept, hostlib.remove_statistical_outliers(xyz, 50, 1.0))
    assert not np.isin([len(xyz) - 2, len(xyz) - 1], kept[0]).any()  # the far pair leaves


def test_report_is_refused_for_a_cloud_the_last_run_did_not_see(ctx):
    """the counts are carried to original indices through the grid of the cloud the context holds: after an upload the last run's
    report is gone (GPD_ERR_STATE), as on a context that never ran one; a buffer too small for the run is GPD_ERR_INVALID"""
    import ctypes
    flat = K.flat_cloud()
    ctx.upload_cloud(flat, np.zeros_like(flat))
    ctx.estimate_normals(K.RADIUS)
    assert ctx.normals_routes()[1]["points"] == len(flat)
    small, info = (ctypes.c_int32 * 8)(), (ctypes.c_longlong * 8)()
    assert api.lib().gpd_hip_last_normals_routes(ctx._h, small, 8, info) == -1
    assert b"room for 8 points, the last run had 2000" in api.lib().gpd_hip_last_error()
    ctx.upload_cloud(flat[:500].copy(), np.zeros_like(flat[:500]))
    with pytest.raises(api.GpdHipError, match="no gpd_hip_estimate_normals ran on the cloud"):
        ctx.normals_routes()
    fresh = api.Context(api.default_params(15))
    try:
        with pytest.raises(api.GpdHipError, match="no gpd_hip_estimate_normals ran on the cloud"):
            fresh.normals_routes()
    finally:
        fresh.close()


def test_independent_float64_form(small_run):
    """Not the oracle's arithmetic: float64 centroid and covariance of the brute-force neighbours, numpy.linalg.eigh.  Where the
    reference's relative gap (l_mid - l_min) / l_max is at least 1e-4 the eigenvector is determined to 10 n 2^-52 / 1e-4 <= 1.8e-7 rad
    (n <= 8193) whatever the summation order, and three float32 components round by sqrt(3) 2^-24 = 1.0e-7: asserted <= 1e-6 rad.
    Largest angle seen on the device: see the printed line (PR text)."""
    r = small_run
    ref, gap = K.eigh_normals(r["xyz"], K.RADIUS)
    ok = gap >= 1e-4
    assert (~ok).sum() <= 0.05 * len(gap)
    g = r["got"].astype(np.float64)
    g /= np.linalg.norm(g, axis=1)[:, None]
    angle = np.arctan2(np.linalg.norm(np.cross(g, ref), axis=1), np.abs((g * ref).sum(1)))
    print("float64 form: %d of %d points compared, smallest gap %.3g, largest angle %.3g rad" % (ok.sum(), len(ok), gap[ok].min(), angle[ok].max()))
    assert angle[ok].max() <= 1e-6
    assert np.abs(np.linalg.norm(r["got"], axis=1) - 1).max() < 1e-6
    towards = (r["got"].astype(np.float64) * (r["vp"][0] - r["xyz"].astype(np.float64))).sum(1)
    assert (towards[np.abs(towards) > 1e-6] > 0).all() and (np.abs(towards) > 1e-6).sum() > 0.9 * len(towards)
