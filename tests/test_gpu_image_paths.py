"""Every route through the image stage (images.hip images_launch) against the oracle, with proof that it ran.

The image stage does not send each candidate through one kernel: the two-per-CU kernels queue the candidates they
cannot hold on device lists, and the large / general instantiations redo those.  A test that only compares pixels stays
green when a rework stops a scene from reaching a fallback, so every test here reads the route report
(gpd_hip_last_image_routes) and asserts three things: the route really ran — for the overflow routes for SOME BUT NOT ALL
candidates of the launch, so that the fast and the slow path share it —, the images equal oracle.images byte for byte
with the same candidate indices, and a second identical call returns the same bytes (the lists fill in atomic order).
The caps come from the report, not from constants copied here."""
import functools

import numpy as np
import pytest
from scipy.spatial import cKDTree

from gpd_amd import api, synth

pytestmark = pytest.mark.gpu

BIT_SHADOW_BIG, BIT_SHADOW_ANY, BIT_POINTS_BIG = 1, 2, 4
FLAG_POINTS, FLAG_VOXELS = 2, 4

# image volumes of the three window classes (image_model.h image::window_class, called by image_state.hip images_reserve)
WIDE = dict(volume_width=0.16, volume_height=0.028)  # box diagonal 0.180 m: 63 of the 64 voxels of a wide window
HUGE = dict(volume_width=0.16, volume_depth=0.10)    # box diagonal 0.193 m: beyond the wide windows
HUGE_DEEP = dict(volume_width=0.30, volume_depth=0.20, volume_height=0.10)  # 0.3 x 0.2 x 0.2 m boxes, 444k voxel cells


def _params(mod, C=15, **kw):
    p = mod.default_params(C)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@functools.lru_cache(maxsize=None)
def _dense_cloud(copies, radius=0.06):
    """synth cloud 1234 (30k points) with `copies` jittered duplicates of every point within `radius` of one object point:
    image boxes there hold `copies + 1` times the points and up to every voxel of the box in shadow.  Returns the cloud,
    the xyz / normals / camera arrays, the object points near the centre and the object points far from it."""
    cl = synth.make_cloud(1234, 30000)
    obj = np.flatnonzero(cl["is_object"])
    t = cKDTree(cl["xyz"].astype(np.float64))
    centre = cl["xyz"][obj[len(obj) // 2]].astype(np.float64)
    ball = np.array(t.query_ball_point(centre, radius))
    rng = np.random.RandomState(3)
    extra = [(cl["xyz"][ball] + rng.uniform(-0.0012, 0.0012, (len(ball), 3))).astype(np.float32) for _ in range(copies)]
    xyz = np.concatenate([cl["xyz"]] + extra)
    nrm = np.concatenate([cl["normals"]] + [cl["normals"][ball]] * copies)
    cam = np.ones((1, len(xyz)), np.int32)
    near = np.array([i for i in t.query_ball_point(centre, 0.045) if cl["is_object"][i]], np.int32)
    d = np.linalg.norm(cl["xyz"][obj].astype(np.float64) - centre, axis=1)
    far = obj[d > 0.3].astype(np.int32)
    return cl, xyz, nrm, cam, near, far


def _pick(idx, n, seed):
    return idx[np.random.RandomState(seed).choice(len(idx), min(n, len(idx)), replace=False)].astype(np.int32)


def _sparse_cloud(seed=1234, step=6):
    """Every `step`-th point of a synth cloud: few shadow voxels per box."""
    cl = synth.make_cloud(seed, 30000)
    keep = np.arange(0, len(cl["xyz"]), step)
    xyz, nrm = cl["xyz"][keep], cl["normals"][keep]
    obj = np.flatnonzero(cl["is_object"][keep]).astype(np.int32)
    return cl, xyz, nrm, np.ones((1, len(xyz)), np.int32), obj


def _routes(ctx, n):
    route, info = ctx.image_routes()
    assert info["candidates"] == n == len(route), (info, n)
    assert ((route & ~7) == 0).all()
    return route, info


def _images(ctx, oracle_mod, p, xyz, nrm, cam, vp, si):
    """search on the context and in the oracle (records byte for byte), then the workspace filter's candidates through
    ctx.images twice and oracle.images -> (images, cand, route, info)."""
    hands = ctx.search(si)
    ohands = oracle_mod.search(p, xyz, nrm, si)
    a, b = hands.copy(), ohands.copy()
    a["score"] = 0
    b["score"] = 0
    assert a.tobytes() == b.tobytes()
    fw = oracle_mod.filter_workspace(p, ohands.copy())
    n = int(fw["valid"].astype(bool).sum())
    assert n > 0
    img, cand = ctx.images(fw)
    route, info = _routes(ctx, n)
    oimg, ocand = oracle_mod.images(p, xyz, nrm, cam, vp, fw)
    assert np.array_equal(cand, ocand)
    assert img.tobytes() == oimg.tobytes()
    img2, cand2 = ctx.images(fw)
    route2, info2 = _routes(ctx, n)
    assert np.array_equal(cand2, cand) and img2.tobytes() == img.tobytes()
    assert np.array_equal(route2, route) and info2 == info
    return img, cand, fw, route, info


def _some_not_all(route, bit):
    k = int(((route & bit) != 0).sum())
    assert 0 < k < len(route), (bit, k, len(route))
    return k


def _box_points(xyz64, tree, h, p, slack):
    """Points of the image neighbourhood (radius nn_radius_images around the sample, grasp_image_body's list) inside the
    hand's image box, in the hand frame in float64: box and radius shrunk (slack < 0) or grown (slack > 0) by |slack|.
    -> (in-box count, neighbourhood size)."""
    r = max(p.volume_depth, p.volume_height / 2.0, p.volume_width)
    idx = tree.query_ball_point(h["sample"], r * (1.0 + 1e-6 * np.sign(slack)))
    t = (xyz64[idx] - h["sample"]) @ h["frame"].reshape(3, 3)
    lo = np.array([h["bottom"], h["center"] - p.volume_width / 2.0, -p.volume_height]) - slack
    hi = np.array([h["bottom"] + p.volume_depth, h["center"] + p.volume_width / 2.0, p.volume_height]) + slack
    return int(((t > lo) & (t < hi)).all(axis=1).sum()), len(idx)


def test_headline_path_takes_no_fallback(oracle_mod, cloud30k):
    """bench.py's workload (configs[1]: the 30k cloud, 15 channels, default windows): every box through the two-per-CU shadow
    kernel, the default shadow set mode.  A few boxes of this cloud hold more than PT_CAP points (2 of ~330 here, ~10 of the
    benchmark's 5000): those, and only those, go to the large points kernel, as an independent count says."""
    p = oracle_mod.default_params(15)
    si = synth.sample_indices(cloud30k, 150)
    ctx = api.Context(api.default_params(15))
    try:
        ctx.upload_cloud(cloud30k["xyz"], cloud30k["normals"], cloud30k["cam_source"], cloud30k["view_points"])
        img, cand, fw, route, info = _images(ctx, oracle_mod, p, cloud30k["xyz"], cloud30k["normals"], cloud30k["cam_source"],
                                             cloud30k["view_points"], si)
        assert len(route) > 200
        assert not (route & (BIT_SHADOW_BIG | BIT_SHADOW_ANY)).any(), np.flatnonzero(route)
        assert info["window_class"] == 0 and info["set_mode"] == 0 and info["status"] == 0
        assert info["pt_cap"] < info["pt_cap_big"] and info["sh_cap"] < info["sh_cap_big"]
        big = np.flatnonzero(route & BIT_POINTS_BIG)
        assert len(big) <= len(route) // 50, big
        x64 = cloud30k["xyz"].astype(np.float64)
        tree = cKDTree(x64)
        for j, h in enumerate(fw.reshape(-1)[cand]):
            if _box_points(x64, tree, h, p, -1e-7)[0] > info["pt_cap"]:
                assert j in big, j
            elif _box_points(x64, tree, h, p, 1e-7)[0] <= info["pt_cap"]:
                assert j not in big, j
    finally:
        ctx.close()


def test_large_shadow_instantiation_default_windows(oracle_mod):
    """Default windows (42 of 42 voxels of reach): boxes under a locally eleven-fold surface hold more shadow voxels than
    shadow_image_kernel<SH_CAP> lists (an estimate with random draws: ~4 % of these candidates at 7000-7500 voxels of the
    ~8900 cells of a box) — shadow_image_kernel<SH_CAP_BIG, false> redoes them, in the same launch as the others."""
    p = oracle_mod.default_params(15)
    cl, xyz, nrm, cam, near, far = _dense_cloud(10, 0.1)
    si = _pick(near, 60, 9)
    ctx = api.Context(api.default_params(15))
    try:
        ctx.upload_cloud(xyz, nrm, cam, cl["view_points"])
        img, cand, fw, route, info = _images(ctx, oracle_mod, p, xyz, nrm, cam, cl["view_points"], si)
        k = _some_not_all(route, BIT_SHADOW_BIG)
        assert not (route & BIT_SHADOW_ANY).any()
        assert info["window_class"] == 0 and info["set_mode"] == 0 and info["status"] == 0
        assert (img[..., 4] > 0).any()
        print("large shadow instantiation: %d of %d candidates" % (k, len(route)))
    finally:
        ctx.close()


@pytest.mark.parametrize("C", [15, 1, 3, 12])
def test_large_points_kernel(oracle_mod, C):
    """Boxes with more than PT_CAP in-box points (a locally six-fold surface) beside ordinary ones (samples far from it):
    grasp_image_kernel<true> redoes the former — on the side stream for 15 channels, on the main stream otherwise.  The
    queue is also checked against an independent float64 count of the points the kernel walks."""
    p = oracle_mod.default_params(C)
    cl, xyz, nrm, cam, near, far = _dense_cloud(5)
    si = np.concatenate([_pick(near, 20, 9), _pick(far, 20, 11)])
    ctx = api.Context(api.default_params(C))
    try:
        ctx.upload_cloud(xyz, nrm, cam, cl["view_points"])
        img, cand, fw, route, info = _images(ctx, oracle_mod, p, xyz, nrm, cam, cl["view_points"], si)
        k = _some_not_all(route, BIT_POINTS_BIG)
        assert info["status"] == 0 and info["window_class"] == 0
        if C != 15:
            assert not (route & (BIT_SHADOW_BIG | BIT_SHADOW_ANY)).any() and info["set_mode"] == -1
        x64 = xyz.astype(np.float64)
        tree = cKDTree(x64)
        flat = fw.reshape(-1)
        decided = 0
        for j, h in enumerate(flat[cand]):
            inner, _ = _box_points(x64, tree, h, p, -1e-7)
            outer, nb = _box_points(x64, tree, h, p, 1e-7)
            if inner > info["pt_cap"]:
                assert route[j] & BIT_POINTS_BIG, (j, inner)
                decided += 1
            elif outer <= info["pt_cap"] and nb <= 65536:
                assert not route[j] & BIT_POINTS_BIG, (j, outer)
                decided += 1
        assert decided > len(cand) // 2, (decided, len(cand))  # a count within 1e-7 m of the cap is left undecided
        print("C=%d: large points kernel for %d of %d candidates" % (C, k, len(route)))
    finally:
        ctx.close()


def test_wide_windows_both_overflow_steps(oracle_mod):
    """Wide windows (0.16 x 0.06 x 0.056 m boxes, ~20.5k voxel cells): under a locally eleven-fold surface many boxes hold
    more than SH_CAP shadow voxels (the large wide instantiation) and a few more than SH_CAP_BIG (queued again, for
    shadow_image_any_kernel) — an estimate with random draws put 2 of 82 candidates at ~12.9k; shadow_set_kernel<1>."""
    p = _params(oracle_mod, 15, **WIDE)
    cl, xyz, nrm, cam, near, far = _dense_cloud(10, 0.1)
    si = np.concatenate([_pick(near, 70, 9), _pick(far, 10, 11)])
    gp = api.default_params(15)
    for k, v in WIDE.items():
        setattr(gp, k, v)
    ctx = api.Context(gp)
    try:
        ctx.upload_cloud(xyz, nrm, cam, cl["view_points"])
        img, cand, fw, route, info = _images(ctx, oracle_mod, p, xyz, nrm, cam, cl["view_points"], si)
        assert info["window_class"] == 1 and info["set_mode"] == 1 and info["status"] == 0
        k1 = _some_not_all(route, BIT_SHADOW_BIG)
        k2 = _some_not_all(route, BIT_SHADOW_ANY)
        assert (route[(route & BIT_SHADOW_ANY) != 0] & BIT_SHADOW_BIG).all()  # queued again = queued once before
        print("wide: large instantiation %d, general kernel %d of %d candidates" % (k1, k2, len(route)))
    finally:
        ctx.close()


def test_huge_windows_general_kernel_for_all(oracle_mod):
    """An image volume beyond the wide windows: shadow_set_kernel<2> and shadow_image_any_kernel for every candidate (no
    queue: the route report is all zero, window class 2)."""
    p = _params(oracle_mod, 15, **HUGE)
    cl = synth.make_cloud(4242, 20000)
    si = synth.sample_indices(cl, 40)
    gp = api.default_params(15)
    for k, v in HUGE.items():
        setattr(gp, k, v)
    ctx = api.Context(gp)
    try:
        ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
        img, cand, fw, route, info = _images(ctx, oracle_mod, p, cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"], si)
        assert len(route) > 20
        assert info["window_class"] == 2 and info["set_mode"] == 2 and info["status"] == 0
        assert not (route & (BIT_SHADOW_BIG | BIT_SHADOW_ANY)).any()
    finally:
        ctx.close()


def _refused(ctx, call, flag):
    with pytest.raises(api.GpdHipError, match="capacity"):
        call()
    route, info = ctx.image_routes()
    assert info["status"] == flag, info  # the text lists every flag: the flag word says which one fired


def test_box_beyond_pt_cap_big_is_refused(oracle_mod, lenet15_real):
    """A locally 81-fold surface puts more than PT_CAP_BIG points into some boxes (~36k at 61-fold by a float64 count):
    images() and detect() raise GPD_ERR_CAPACITY with exactly flag 2 — never truncated images.  The same context then
    images an ordinary cloud equal to the oracle."""
    p = oracle_mod.default_params(15)
    cl, xyz, nrm, cam, near, far = _dense_cloud(80)
    si = _pick(near, 12, 9)
    ctx = api.Context(api.default_params(15))
    try:
        ctx.set_lenet_weights(lenet15_real)
        ctx.upload_cloud(xyz, nrm, cam, cl["view_points"])
        hands = ctx.search(si)
        fw = oracle_mod.filter_workspace(p, oracle_mod.search(p, xyz, nrm, si))
        assert hands.shape == fw.shape
        x64 = xyz.astype(np.float64)
        tree = cKDTree(x64)
        counts = [_box_points(x64, tree, h, p, -1e-7)[0] for h in fw.reshape(-1)[fw.reshape(-1)["valid"].astype(bool)]]
        _, info = ctx.image_routes()
        assert max(counts) > info["pt_cap_big"], max(counts)
        _refused(ctx, lambda: ctx.images(fw), FLAG_POINTS)
        _refused(ctx, lambda: ctx.detect(si), FLAG_POINTS)
        sp = _sparse_cloud()
        ctx.upload_cloud(sp[1], sp[2], sp[3], sp[0]["view_points"])
        _, _, _, route, info = _images(ctx, oracle_mod, p, sp[1], sp[2], sp[3], sp[0]["view_points"], _pick(sp[4], 30, 5))
        assert info["status"] == 0 and not route.any()
    finally:
        ctx.close()


def test_box_beyond_huge_cap_voxels_is_refused(oracle_mod, lenet15_real):
    """HUGE_CAP (65535 shadow voxels in one box) inside the 0.77 m window: 0.3 x 0.2 x 0.2 m boxes (window edge 141 voxels)
    hold 444k voxel cells, and on the 30k cloud the shadow of the surface fills 70-110k of them (estimate with random
    draws) — images() and detect() raise with exactly flag 4.  Every sixth point of the cloud leaves 4-40k voxels per box:
    the same context then images that equal to the oracle."""
    p = _params(oracle_mod, 15, **HUGE_DEEP)
    gp = api.default_params(15)
    for k, v in HUGE_DEEP.items():
        setattr(gp, k, v)
    cl = synth.make_cloud(1234, 30000)
    si = synth.sample_indices(cl, 10)
    ctx = api.Context(gp)
    try:
        ctx.set_lenet_weights(lenet15_real)
        ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
        ctx.search(si)
        fw = oracle_mod.filter_workspace(p, oracle_mod.search(p, cl["xyz"], cl["normals"], si))
        assert fw["valid"].any()
        _refused(ctx, lambda: ctx.images(fw), FLAG_VOXELS)
        _refused(ctx, lambda: ctx.detect(si), FLAG_VOXELS)
        sp = _sparse_cloud()
        ctx.upload_cloud(sp[1], sp[2], sp[3], sp[0]["view_points"])
        _, _, _, route, info = _images(ctx, oracle_mod, p, sp[1], sp[2], sp[3], sp[0]["view_points"], _pick(sp[4], 12, 5))
        assert info["status"] == 0 and info["window_class"] == 2 and not (route & (BIT_SHADOW_BIG | BIT_SHADOW_ANY)).any()
    finally:
        ctx.close()


@pytest.mark.parametrize("volume", ["default", "wide"])
def test_stale_shadow_rows_between_launches(oracle_mod, volume):
    """shadow_set_kernel<0> writes only the rows its candidates' windows cover; the rest of a set's bitset keeps what an
    earlier launch left.  One context: dense cloud A (many shadow voxels), sparse cloud B (its first hand sets land on
    A's set rows), A again — each equal to the oracle and to a fresh context's bytes; the route report after B is all zero."""
    kw = WIDE if volume == "wide" else {}
    p = _params(oracle_mod, 15, **kw)
    gp = api.default_params(15)
    for k, v in kw.items():
        setattr(gp, k, v)
    cl, xyz, nrm, cam, near, far = _dense_cloud(10, 0.1)
    si_a = _pick(near, 30, 9)
    sp = _sparse_cloud(4242)
    si_b = _pick(sp[4], 40, 5)
    A = (xyz, nrm, cam, cl["view_points"], si_a)
    B = (sp[1], sp[2], sp[3], sp[0]["view_points"], si_b)

    def run(ctx, scene):
        ctx.upload_cloud(*scene[:4])
        return _images(ctx, oracle_mod, p, *scene)

    ctx = api.Context(gp)
    try:
        a1 = run(ctx, A)
        b = run(ctx, B)
        assert not b[3].any() and b[4]["status"] == 0
        a2 = run(ctx, A)
        assert a2[0].tobytes() == a1[0].tobytes() and np.array_equal(a2[3], a1[3])
    finally:
        ctx.close()
    fresh = api.Context(gp)
    try:
        fb = run(fresh, B)
        assert fb[0].tobytes() == b[0].tobytes() and np.array_equal(fb[1], b[1])
    finally:
        fresh.close()
