"""grasp_image_kernel<true> walks its queue in (candidate, projection) items, and shadow_set_kernel<0> drops the rays that
cannot reach the voxel bounding box of its candidates' windows and packs the others inside the wave before it draws them
(images.hip).  Every case here is compared with oracle.images byte for byte; that the case is the one it is meant to be —
the length of the queue, a set none of whose rays reaches a window, ray components that are exactly zero, a window on the
region's outermost rows, the neighbourhood sizes — is established on the CPU, from the route report, the fallback counters
and float64 arithmetic of its own."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import given_cases as gc
from gpd_amd import api, synth
from test_gpu_image_paths import BIT_POINTS_BIG, FLAG_POINTS, _box_points, _dense_cloud, _pick, _routes

pytestmark = pytest.mark.gpu

LGRID = 256        # workgroups of the large instantiations (image_model.h)
SET_THREADS = 1024  # threads of shadow_set_kernel: one ray each per round
VOXEL = 0.003
SD, SR = 86, 43    # the default set region: offsets -43 .. 42 from the sample's voxel
LCG_BASE = 12345678901
SHADOW = [4, 9, 14]


def _upload(ctx, cl):
    ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])


def _radius(p):
    return max(p.volume_depth, p.volume_height / 2.0, p.volume_width)


def _only(fw, cand, keep):
    """fw with every validity flag cleared but those of the candidates cand[keep]"""
    out = fw.copy()
    flat = out.reshape(-1)
    mask = np.zeros(len(flat), bool)
    mask[cand[keep]] = True
    flat["valid"][~mask] = 0
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the overflow queue of the points kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [15, 12, 3, 1])
def test_overflow_queue_of_one_then_another_list(oracle_mod, C):
    """Every image layout (3, 3, 1 and 1 projections per candidate).  One context, three lists: all candidates of a locally
    six-fold surface (some boxes beyond PT_CAP, not compared: it only finds them), then ONE of those beside ordinary
    candidates — a queue of exactly one entry, so 3 (or 1) items —, then all the queued ones and nothing else."""
    p = oracle_mod.default_params(C)
    cl, xyz, nrm, cam, near, far = _dense_cloud(5)
    si = np.concatenate([_pick(near, 20, 9), _pick(far, 20, 11)])
    ctx = api.Context(api.default_params(C))
    try:
        ctx.upload_cloud(xyz, nrm, cam, cl["view_points"])
        fw = oracle_mod.filter_workspace(p, ctx.search(si).copy())
        _, cand = ctx.images(fw, download=False)
        route, info = _routes(ctx, len(cand))
        big = np.flatnonzero(route & BIT_POINTS_BIG)
        small = np.flatnonzero((route & BIT_POINTS_BIG) == 0)
        assert info["status"] == 0 and len(big) >= 3 and len(small) >= 20, (len(big), len(small))
        assert ctx.fallbacks()["large_points_kernel_candidates"] == len(big)
        for keep, want_big in ((np.concatenate([big[len(big) // 2:][:1], small[::3]]), 1), (big, len(big))):
            lst = _only(fw, cand, keep)
            img, c2 = ctx.images(lst)
            r2, i2 = _routes(ctx, len(c2))
            assert i2["status"] == 0 and len(c2) == len(keep)
            assert int(((r2 & BIT_POINTS_BIG) != 0).sum()) == want_big == ctx.fallbacks()["large_points_kernel_candidates"]
            oimg, ocand = oracle_mod.images(p, xyz, nrm, cam, cl["view_points"], lst)
            assert np.array_equal(c2, ocand) and img.shape[1:] == (60, 60, C)
            bad = np.flatnonzero((img != oimg).reshape(len(c2), -1).any(axis=1))
            assert img.tobytes() == oimg.tobytes(), (bad, r2[bad])
        print("C=%d: %d of %d candidates beyond PT_CAP" % (C, len(big), len(cand)))
    finally:
        ctx.close()


def test_overflow_queue_longer_than_the_grid_twelve_channels(oracle_mod):
    """150 samples under a locally eleven-fold surface queue more candidates than grasp_image_kernel<true> has workgroups
    (444 at 15 channels: 1332 items on 256 workgroups, five or six in a row in one LDS and one scratch row).  The second
    launch images exactly the queued ones, so that the oracle has those to make and not all."""
    C = 12
    p = oracle_mod.default_params(C)
    cl, xyz, nrm, cam, near, far = _dense_cloud(10, 0.1)
    si = np.concatenate([_pick(near, 150, 9), _pick(far, 4, 11)])
    ctx = api.Context(api.default_params(C))
    try:
        ctx.upload_cloud(xyz, nrm, cam, cl["view_points"])
        fw = oracle_mod.filter_workspace(p, ctx.search(si).copy())
        _, cand = ctx.images(fw, download=False)
        route, info = _routes(ctx, len(cand))
        big = np.flatnonzero(route & BIT_POINTS_BIG)
        assert info["status"] == 0 and LGRID < len(big) < len(cand), (len(big), len(cand))
        lst = _only(fw, cand, big)
        img, c2 = ctx.images(lst)
        r2, i2 = _routes(ctx, len(c2))
        assert i2["status"] == 0 and len(c2) == len(big) and (r2 & BIT_POINTS_BIG).all()
        assert ctx.fallbacks()["large_points_kernel_candidates"] == len(big)
        oimg, ocand = oracle_mod.images(p, xyz, nrm, cam, cl["view_points"], lst)
        assert np.array_equal(c2, ocand) and img.tobytes() == oimg.tobytes()
        print("%d candidates = %d items on %d workgroups" % (len(big), 3 * len(big), LGRID))
    finally:
        ctx.close()


def test_box_beyond_pt_cap_big_is_reported_once_per_candidate(oracle_mod):
    """A locally 81-fold surface: some boxes hold more than PT_CAP_BIG points.  Each of their three items finds that out;
    the launch still raises with exactly the points flag, and the queue counter is the number of candidates beyond PT_CAP
    by a float64 count — not a multiple of it."""
    p = oracle_mod.default_params(15)
    cl, xyz, nrm, cam, near, far = _dense_cloud(80)
    si = _pick(near, 12, 9)
    ctx = api.Context(api.default_params(15))
    try:
        ctx.upload_cloud(xyz, nrm, cam, cl["view_points"])
        fw = oracle_mod.filter_workspace(p, ctx.search(si).copy())
        with pytest.raises(api.GpdHipError, match="capacity"):
            ctx.images(fw)
        route, info = ctx.image_routes()
        assert info["status"] == FLAG_POINTS, info
        x64 = xyz.astype(np.float64)
        tree = cKDTree(x64)
        flat = fw.reshape(-1)
        valid = flat[flat["valid"].astype(bool)]
        assert len(valid) == info["candidates"]
        inner = np.array([_box_points(x64, tree, h, p, -1e-7)[0] for h in valid])
        outer = np.array([_box_points(x64, tree, h, p, 1e-7)[0] for h in valid])
        assert (inner > info["pt_cap_big"]).sum() >= 1
        queued = ctx.fallbacks()["large_points_kernel_candidates"]
        assert (inner > info["pt_cap"]).sum() <= queued <= (outer > info["pt_cap"]).sum(), (queued, len(valid))
        assert int(((route & BIT_POINTS_BIG) != 0).sum()) == queued
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# the rays of shadow_set_kernel<0>
# ---------------------------------------------------------------------------------------------------------------------
def _neighbours(oracle_mod, cl, sample, p):
    return np.asarray(oracle_mod.radius_search(cl["xyz"], np.asarray(sample, np.float64), _radius(p))[0])


def _given_equal(oracle_mod, ctx, cl, hands, base=0):
    """ctx.images_given against oracle.images at the stream position `base` -> images"""
    op = oracle_mod.default_params(15)
    oracle_mod.set_lcg_base(base)
    try:
        wimg, wcand = oracle_mod.images(op, cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"], hands)
        wdraws = oracle_mod.last_lcg_draws()
    finally:
        oracle_mod.set_lcg_base(0)
    gimg, gcand, gdraws = ctx.images_given(hands, lcg_base=base)
    route, info = ctx.image_routes()
    assert info["status"] == 0 and info["set_mode"] == 0 and info["window_class"] == 0, info
    assert np.array_equal(gcand, wcand) and gdraws == wdraws and len(wcand) > 0
    bad = np.flatnonzero((gimg != wimg).reshape(len(wcand), -1).any(axis=1))
    assert gimg.tobytes() == wimg.tobytes(), (len(bad), bad[:10])
    return gimg


@pytest.fixture(scope="module")
def scene():
    """6000 points, one camera at the origin, 12 samples, and the records ctx.search returns for them"""
    cl, si = gc.scene(two_cameras=False)
    si = si[:12]
    ctx = api.Context(api.default_params(15))
    try:
        _upload(ctx, cl)
        hands = ctx.search(si)
    finally:
        ctx.close()
    hands.setflags(write=False)
    return cl, si, hands


def _rot_to(d, e):
    """rotation that takes the unit vector d to the unit vector e"""
    ax = np.cross(d, e)
    s = np.linalg.norm(ax)
    if s < 1e-12:
        return np.eye(3) if d @ e > 0 else gc._rotation(np.cross(d, [0.3, 0.5, 0.8]), np.pi)
    return gc._rotation(ax, np.arctan2(s, d @ e))


def _set_of(template, sample, frames, bottom, center):
    """one hand set [1, slots]: the template's records with this sample, these frames (columns = hand axes), all valid"""
    h = template.copy().reshape(1, -1)
    for j in range(h.shape[1]):
        h[0, j]["sample"] = sample
        h[0, j]["frame"] = np.asarray(frames[j], np.float64).ravel()
        h[0, j]["bottom"] = bottom
        h[0, j]["center"] = center[j] if np.ndim(center) else center
        h[0, j]["valid"] = 1
        h[0, j]["score"] = 0.0
    return h


def test_set_whose_rays_all_run_away_from_its_boxes(oracle_mod, scene):
    """Samples lifted 85 mm off the surface towards the camera, the hands' boxes on the camera's side of them: every
    neighbourhood point lies 15 mm or more behind the plane the boxes start at, and every ray runs further away — no ray
    reaches the bounding box of the windows, none is drawn.  The shadow planes are the oracle's: empty."""
    cl, si, hands = scene
    p = oracle_mod.default_params(15)
    x64 = cl["xyz"].astype(np.float64)
    vp = cl["view_points"][0].astype(np.float64)
    sets = []
    for s in range(len(si)):
        u = vp - x64[si[s]]
        u /= np.linalg.norm(u)
        smp = x64[si[s]] + 0.085 * u
        nb = _neighbours(oracle_mod, cl, smp, p)
        if len(nb) < 8:
            continue
        depth = (x64[nb] - smp) @ u
        vec = x64[nb].mean(axis=0) - vp  # the direction of the rays: away from the camera
        if depth.max() > -0.015 or vec @ u >= 0:
            continue
        a = np.cross(u, [0.0, 0.0, 1.0])
        a /= np.linalg.norm(a)
        F0 = np.stack([u, a, np.cross(u, a)], axis=1)
        frames = [gc._rotation(u, k * np.pi / 8) @ F0 for k in range(hands.shape[1])]
        sets.append(_set_of(hands[s], smp, frames, 0.0, np.linspace(-0.05, 0.05, hands.shape[1])))
    assert len(sets) >= 4, len(sets)
    f = np.ascontiguousarray(np.concatenate(sets))
    assert api.given_check(api.default_params(15), f) is None
    ctx = api.Context(api.default_params(15))
    try:
        _upload(ctx, cl)
        img = _given_equal(oracle_mod, ctx, cl, f)
        assert (img[..., SHADOW] == 0).all()
        # the same sets seen from behind the surface: the rays run through the boxes, the shadow planes are not empty
        back = dict(cl, view_points=np.ascontiguousarray((2.0 * x64[si].mean(axis=0) - vp)[None, :]))
        _upload(ctx, back)
        img2 = _given_equal(oracle_mod, ctx, back, f)
        assert (img2[..., SHADOW] > 0).any()
    finally:
        ctx.close()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_view_point_on_a_coordinate_axis_through_the_centre(oracle_mod, axis):
    """Coordinates on a 2^-12 m lattice make the neighbourhood's mean exact in any order of summation, so a view point that
    differs from it in one coordinate only gives a ray direction with two components exactly zero: the rays are parallel
    to two of the three slabs they are tested against."""
    p = oracle_mod.default_params(15)
    cl = synth.make_cloud(77, 3000)
    xyz = (np.round(cl["xyz"].astype(np.float64) * 4096.0) / 4096.0).astype(np.float32)
    assert np.array_equal(xyz.astype(np.float64) * 4096.0, np.round(xyz.astype(np.float64) * 4096.0))
    cl = dict(cl, xyz=xyz)
    si = synth.sample_indices(cl, 3)[1:2]
    nb = _neighbours(oracle_mod, cl, xyz[si[0]], p)
    assert 64 < len(nb) < 2 ** 20
    centre = xyz[nb].astype(np.float64).sum(axis=0) / float(len(nb))  # (sums of < 2^20 multiples of 2^-12 below 2: exact)
    vp = centre.copy()
    vp[axis] += 0.7
    vec = centre - vp
    assert (vec != 0).sum() == 1 and vec[axis] != 0
    cl = dict(cl, view_points=np.ascontiguousarray(vp[None, :]), cam_source=np.ones((1, len(xyz)), np.int32))
    ctx = api.Context(api.default_params(15))
    try:
        _upload(ctx, cl)
        hands = ctx.search(si)
        fw = oracle_mod.filter_workspace(p, hands.copy())
        assert fw["valid"].any()
        img, cand = ctx.images(fw)
        route, info = _routes(ctx, len(cand))
        assert info["status"] == 0 and info["set_mode"] == 0
        oimg, ocand = oracle_mod.images(p, cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"], fw)
        assert np.array_equal(cand, ocand) and img.tobytes() == oimg.tobytes()
        assert (img[..., SHADOW] > 0).any()
    finally:
        ctx.close()


def test_windows_on_the_outermost_rows_of_the_region(oracle_mod, scene):
    """Six sets whose boxes reach as far from the sample as the default hand allows (the corner at bottom 0, center 0.055:
    40.9 voxels), turned so that this corner lies on +x, -x, +y, -y, +z, -z; the samples sit in the middle of their voxel.
    The window of such a box ends on row 85 = SD - 1 of the set's region, or begins on row 1 (the region keeps one spare
    row on the low side): the bounding box the rays are tested against is clamped to the region there.  Also at another
    position of the stream of draws (lcg_base != 0, as gpd_hip_detect_sharded sets it)."""
    cl, si, hands = scene
    p = oracle_mod.default_params(15)
    x64 = cl["xyz"].astype(np.float64)
    corner = np.array([p.volume_depth, 0.055 + p.volume_width / 2.0, p.volume_height])
    d = corner / np.linalg.norm(corner)
    sets, want = [], []
    for k in range(6):
        e = np.zeros(3)
        e[k // 2] = 1.0 if k % 2 == 0 else -1.0
        smp = (np.floor(x64[si[k]] / VOXEL) + 0.5) * VOXEL
        R = _rot_to(d, e)
        frames = [gc._rotation(e, j * np.pi / 4) @ R for j in range(hands.shape[1])]
        sets.append(_set_of(hands[k], smp, frames, 0.0, 0.055))
        # the window of slot 0's box, floor(min) - 1 .. floor(max) + 1, relative to the region (shadow_image_body)
        lo = np.array([0.0, 0.055 - p.volume_width / 2.0, -p.volume_height])
        hi = np.array([p.volume_depth, 0.055 + p.volume_width / 2.0, p.volume_height])
        cs = np.array([[(hi if (c >> a) & 1 else lo)[a] for a in range(3)] for c in range(8)])
        w = smp + cs @ frames[0].T
        org = np.floor(smp * (1.0 / VOXEL)) - SR
        first = np.floor(w.min(axis=0) * (1.0 / VOXEL)) - 1 - org
        last = np.floor(w.max(axis=0) * (1.0 / VOXEL)) + 1 - org
        want.append((int(first[k // 2]), int(last[k // 2])))
        assert len(_neighbours(oracle_mod, cl, smp, p)) > 64
    assert [w[1] for w in want[0::2]] == [SD - 1] * 3 and [w[0] for w in want[1::2]] == [1] * 3, want
    f = np.ascontiguousarray(np.concatenate(sets))
    assert api.given_check(api.default_params(15), f) is None
    ctx = api.Context(api.default_params(15))
    try:
        _upload(ctx, cl)
        img = _given_equal(oracle_mod, ctx, cl, f)
        img_b = _given_equal(oracle_mod, ctx, cl, f, LCG_BASE)
        assert (img[..., SHADOW] > 0).any() and img_b.tobytes() != img.tobytes()
    finally:
        ctx.close()


@pytest.mark.parametrize("every,lo,hi", [(60, 1, 63), (6, 65, 1023), (1, 1025, 4095)])
def test_neighbourhood_sizes_around_the_wave_and_the_round(oracle_mod, scene, every, lo, hi):
    """The records of the 6000-point scene imaged on every 60th of its points (neighbourhoods of fewer than 64 points: not one
    full wave of rays), on every sixth (a few hundred: one round of SET_THREADS rays, most waves with idle lanes) and on
    all of them (more than SET_THREADS and not a multiple: later rounds that only some waves take part in)."""
    cl, si, hands = scene
    p = oracle_mod.default_params(15)
    keep = np.arange(len(cl["xyz"])) % every == 0
    other = dict(xyz=np.ascontiguousarray(cl["xyz"][keep]), normals=np.ascontiguousarray(cl["normals"][keep]),
                 cam_source=np.ascontiguousarray(cl["cam_source"][:, keep]), view_points=cl["view_points"])
    n = np.array([len(_neighbours(oracle_mod, other, hands[s, 0]["sample"], p)) for s in range(len(hands))])
    hit = (n >= lo) & (n <= hi)
    assert hit.sum() >= 3 and (n[hit] % SET_THREADS != 0).all(), n
    f = np.ascontiguousarray(hands[hit])
    assert f["valid"].any()
    ctx = api.Context(api.default_params(15))
    try:
        _upload(ctx, other)
        img = _given_equal(oracle_mod, ctx, other, f)
        if every != 60:
            assert (img[..., SHADOW] > 0).any()
        print("neighbourhoods of", sorted(n[hit]))
    finally:
        ctx.close()


def test_two_cameras_one_of_them_blind_for_some_sets(oracle_mod, scene):
    """Camera 1 sees only the points within 0.02 m of one sample: the sets near it are the intersection of two cameras'
    voxel sets (two bitsets, each with its own ray direction and its own surviving rays), the sets far from it camera
    0's alone."""
    cl, si, hands = scene
    p = oracle_mod.default_params(15)
    x64 = cl["xyz"].astype(np.float64)
    dist = np.linalg.norm(x64 - x64[si[0]], axis=1)
    cam = np.stack([np.ones(len(x64), np.int32), (dist < 0.02).astype(np.int32)])
    two = dict(cl, cam_source=cam, view_points=np.array([cl["view_points"][0], [0.3, -0.2, 0.1]], np.float64))
    seen1 = np.array([cam[1][_neighbours(oracle_mod, two, hands[s, 0]["sample"], p)].any() for s in range(len(hands))])
    assert 1 <= seen1.sum() < len(hands), seen1
    f = np.ascontiguousarray(hands)
    ctx = api.Context(api.default_params(15))
    try:
        _upload(ctx, two)
        img = _given_equal(oracle_mod, ctx, two, f)
        one = dict(two, cam_source=np.ascontiguousarray(cam[:1]), view_points=np.ascontiguousarray(two["view_points"][:1]))
        _upload(ctx, one)
        img1 = _given_equal(oracle_mod, ctx, one, f)
        assert img.tobytes() != img1.tobytes()
    finally:
        ctx.close()
