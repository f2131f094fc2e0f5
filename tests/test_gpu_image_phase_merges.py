"""The per-candidate image kernels (images.hip shadow_image_body / grasp_image_body) ride several pieces of work on a
neighbouring phase's barrier: the pixel counters are cleared by the previous projection's last phase, `max - value` of the
shadow raster is taken inside the dilation's loads (empty pixels are marked, not zero), the list of non-empty pixels is
built inside the scan and the segment-table phase, the background of the staged bytes is written per group.  The
benchmark cloud does not reach the cases in which such a merge can go wrong; these do, each against oracle.images byte
for byte, and each asserts from the route report, the fallback counters and an independent float64 count that the case
it is about really occurred."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

from gpd_amd import api, synth
from test_gpu_image_paths import (BIT_POINTS_BIG, BIT_SHADOW_ANY, BIT_SHADOW_BIG, _box_points, _dense_cloud, _images, _pick,
                                  _routes, _some_not_all)

pytestmark = pytest.mark.gpu

LGRID = 256  # workgroups of the large instantiations (image_model.h): a longer queue gives a workgroup several candidates in a row


def _planes_constant(img):
    """[n, C] bool: is the channel one value over the whole image"""
    f = img.reshape(len(img), -1, img.shape[-1])
    return f.max(1) == f.min(1)


def _live_groups(x64, tree, h, p):
    """(in-box points, per projection the number of 4-pixel groups whose 3 x 6 dilation window holds a point): the cells in
    float64 (image_strategy.cpp:92-102), the group geometry of grasp_image_body."""
    r = max(p.volume_depth, p.volume_height / 2.0, p.volume_width)
    t = (x64[tree.query_ball_point(h["sample"], r)] - h["sample"]) @ h["frame"].reshape(3, 3)
    off = np.array([h["bottom"], h["center"] - p.volume_width / 2.0, -p.volume_height])
    ln = np.array([p.volume_depth, p.volume_width, 2.0 * p.volume_height])
    t = t[((t > off) & (t < off + ln)).all(axis=1)]
    c = np.minimum(np.floor((t - off) / ln * 60).astype(int), 59)
    live = []
    for pr in range(3):
        v = c[:, 0] if pr == 0 else c[:, 2]
        hz = c[:, 0] if pr == 2 else c[:, 1]
        occ = np.zeros((60, 60), bool)
        occ[v, hz] = True
        pad = np.pad(occ, 1)
        d = np.zeros((60, 60), bool)
        for a in range(3):
            for b in range(3):
                d |= pad[a:a + 60, b:b + 60]
        live.append(int(d.reshape(60, 15, 4).any(axis=2).sum()))
    return len(t), live


@pytest.fixture(scope="module")
def small_cloud():
    return synth.make_cloud(77, 3000)


@pytest.mark.parametrize("C", [15, 12, 3, 1])
def test_small_cloud_every_channel_count(oracle_mod, small_cloud, C):
    """3000 points, 24 samples, every image layout: all candidates through the two-per-CU kernels, nothing queued."""
    cl = small_cloud
    p = oracle_mod.default_params(C)
    ctx = api.Context(api.default_params(C))
    try:
        ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
        img, cand, fw, route, info = _images(ctx, oracle_mod, p, cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"],
                                             synth.sample_indices(cl, 24))
        assert len(cand) > 50 and img.shape[1:] == (60, 60, C)
        assert not route.any() and info["status"] == 0 and info["window_class"] == 0
        assert info["set_mode"] == (0 if C == 15 else -1)
        fb = ctx.fallbacks()
        assert fb["large_shadow_kernel_candidates"] == 0 and fb["large_points_kernel_candidates"] == 0
        assert ctx.images_stats()["candidates"] == len(cand)
    finally:
        ctx.close()


def test_candidates_without_a_shadow_bitset(oracle_mod, cloud30k):
    """Two cameras, the first of which sees only the points within 0.15 m of one object point: a hand set whose
    neighbourhood it does not see has no shadow bitset (the shadow is camera 0's set cut with the others', hand_set.cpp:159-172),
    its candidates' shadow kernels list nothing — the maximum over an empty mask is 0 and all three shadow planes are one
    value — beside hand sets with a two-camera shadow in the same launch."""
    cl = cloud30k
    p = oracle_mod.default_params(15)
    x64 = cl["xyz"].astype(np.float64)
    obj = np.flatnonzero(cl["is_object"])
    dist = np.linalg.norm(x64 - x64[obj[len(obj) // 2]], axis=1)
    cam = np.stack([(dist < 0.15).astype(np.int32), np.ones(len(x64), np.int32)])
    vp = np.array([[0.0, 0.0, 0.0], [0.3, -0.2, 0.1]])
    si = np.concatenate([_pick(obj[dist[obj] < 0.04], 8, 9), _pick(obj[dist[obj] > 0.3], 8, 11)])
    ctx = api.Context(api.default_params(15))
    try:
        ctx.upload_cloud(cl["xyz"], cl["normals"], cam, vp)
        img, cand, fw, route, info = _images(ctx, oracle_mod, p, cl["xyz"], cl["normals"], cam, vp, si)
        assert not (route & (BIT_SHADOW_BIG | BIT_SHADOW_ANY)).any() and info["status"] == 0 and info["set_mode"] == 0
        fb = ctx.fallbacks()
        assert fb["large_shadow_kernel_candidates"] == 0
        assert fb["large_points_kernel_candidates"] == int(((route & BIT_POINTS_BIG) != 0).sum())
        assert ctx.images_stats()["candidates"] == len(cand)
        tree = cKDTree(x64)
        r = max(p.volume_depth, p.volume_height / 2.0, p.volume_width)
        unseen = np.array([not (dist[tree.query_ball_point(h["sample"], r * 1.001)] < 0.15).any() for h in fw.reshape(-1)[cand]])
        const = _planes_constant(img)[:, [4, 9, 14]].all(axis=1)
        assert 5 < unseen.sum() < len(cand) - 5, (unseen.sum(), len(cand))
        assert const[unseen].all() and not const[~unseen].any()
        assert (img[unseen][..., [4, 9, 14]] == 0).all()
    finally:
        ctx.close()


THIN = dict(volume_depth=0.01)  # image boxes that keep the first centimetre above the hand's base: many hold nothing


def test_boxes_without_points_and_without_shadow_voxels(oracle_mod, small_cloud):
    """A 1 cm deep image volume: a quarter of the boxes hold no point at all — no non-empty pixel, no live group, every
    group background in all four planes of every projection — and most of those no shadow voxel either although their
    hand set has a bitset, so that every plane of the image is one value; a few boxes hold points but no shadow voxel.
    They run beside ordinary candidates of the same hand sets."""
    cl = small_cloud
    p = oracle_mod.default_params(15)
    gp = api.default_params(15)
    for k, v in THIN.items():
        setattr(p, k, v)
        setattr(gp, k, v)
    ctx = api.Context(gp)
    try:
        ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
        img, cand, fw, route, info = _images(ctx, oracle_mod, p, cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"],
                                             synth.sample_indices(cl, 24))
        assert not route.any() and info["status"] == 0 and info["window_class"] == 0 and info["set_mode"] == 0
        fb = ctx.fallbacks()
        assert fb["large_shadow_kernel_candidates"] == 0 and fb["large_points_kernel_candidates"] == 0
        assert ctx.images_stats()["candidates"] == len(cand)
        x64 = cl["xyz"].astype(np.float64)
        tree = cKDTree(x64)
        flat = fw.reshape(-1)
        empty = np.array([_box_points(x64, tree, h, p, 1e-7)[0] == 0 for h in flat[cand]])  # not even within 1e-7 m of the box
        filled = np.array([_box_points(x64, tree, h, p, -1e-7)[0] > 0 for h in flat[cand]])
        const = _planes_constant(img)
        assert 10 <= empty.sum() < len(cand) // 2, empty.sum()
        assert const[empty][:, [0, 1, 2, 3, 5, 6, 7, 8, 10, 11, 12, 13]].all()  # no point: normals and depth are background
        assert const[empty].all(axis=1).sum() >= 10  # ... and with no shadow voxel in the box: everything
        assert const[filled][:, [4, 9, 14]].all(axis=1).any()  # points, but no shadow voxel
        assert not const[filled].all(axis=1).any()
    finally:
        ctx.close()


def test_every_group_live(oracle_mod):
    """Under a locally eleven-fold surface a box seen along the approach axis has a point in the window of every one of
    the 900 pixel groups: no group is background, the minimum and the maximum come from the dilated values alone (0 takes
    part only where a window holds an empty pixel).  A float64 count finds the candidates; with ~5000 points in the box
    they run in grasp_image_kernel<true>, which shares the body."""
    p = oracle_mod.default_params(15)
    cl, xyz, nrm, cam, near, far = _dense_cloud(10, 0.1)
    si = _pick(near, 12, 9)
    ctx = api.Context(api.default_params(15))
    try:
        ctx.upload_cloud(xyz, nrm, cam, cl["view_points"])
        img, cand, fw, route, info = _images(ctx, oracle_mod, p, xyz, nrm, cam, cl["view_points"], si)
        assert info["status"] == 0
        x64 = xyz.astype(np.float64)
        tree = cKDTree(x64)
        res = [_live_groups(x64, tree, h, p) for h in fw.reshape(-1)[cand]]
        full = [j for j, (n, live) in enumerate(res) if 900 in live]
        assert full and len(full) < len(cand), (len(full), len(cand))
        assert any(max(live) < 900 and n > 0 for n, live in res)
        for j in full:
            assert res[j][0] > info["pt_cap"] and route[j] & BIT_POINTS_BIG
        assert ctx.fallbacks()["large_points_kernel_candidates"] == int(((route & BIT_POINTS_BIG) != 0).sum())
    finally:
        ctx.close()


def test_large_points_kernel_takes_several_candidates_in_a_row(oracle_mod):
    """150 samples under the eleven-fold surface queue more candidates for grasp_image_kernel<true> than it has workgroups:
    a workgroup runs two candidates one after the other in the same LDS (what one leaves in the pixel counters, the
    histogram and the reduction slots is what the next one finds), beside a few boxes that overflow into
    shadow_image_kernel<SH_CAP_BIG>.  (A handful of samples, as in test_every_group_live, keeps every queue shorter than
    the grid.)"""
    p = oracle_mod.default_params(15)
    cl, xyz, nrm, cam, near, far = _dense_cloud(10, 0.1)
    si = np.concatenate([_pick(near, 150, 9), _pick(far, 4, 11)])
    ctx = api.Context(api.default_params(15))
    try:
        ctx.upload_cloud(xyz, nrm, cam, cl["view_points"])
        img, cand, fw, route, info = _images(ctx, oracle_mod, p, xyz, nrm, cam, cl["view_points"], si)
        assert info["status"] == 0 and info["window_class"] == 0
        k = _some_not_all(route, BIT_POINTS_BIG)
        assert k > LGRID, k
        ks = _some_not_all(route, BIT_SHADOW_BIG)
        fb = ctx.fallbacks()
        assert fb["large_points_kernel_candidates"] == k and fb["large_shadow_kernel_candidates"] == ks
        print("large points kernel: %d candidates on %d workgroups, large shadow kernel: %d" % (k, LGRID, ks))
    finally:
        ctx.close()


def test_large_shadow_kernel_takes_several_candidates_in_a_row(oracle_mod):
    """Every object point within 0.17 m of the centre of a 0.2 m ball of eleven-fold surface as a sample: about one
    candidate in twenty holds more than SH_CAP shadow voxels, more of them than shadow_image_kernel<SH_CAP_BIG> has
    workgroups.  The second launch images exactly those candidates (every other validity flag cleared), so that the
    oracle has a few hundred images to make and not thirteen thousand: the queue is again longer than the grid — a
    workgroup runs two or three boxes one after the other in the same LDS: pixel counters, histogram, reduction slots,
    the marked raster — and every image equals the oracle's."""
    p = oracle_mod.default_params(15)
    cl, xyz, nrm, cam, near, far = _dense_cloud(10, 0.2)
    x64 = cl["xyz"].astype(np.float64)
    obj = np.flatnonzero(cl["is_object"])
    si = obj[np.linalg.norm(x64[obj] - x64[obj[len(obj) // 2]], axis=1) < 0.17].astype(np.int32)
    ctx = api.Context(api.default_params(15))
    try:
        ctx.upload_cloud(xyz, nrm, cam, cl["view_points"])
        fw = oracle_mod.filter_workspace(p, ctx.search(si).copy())
        _, cand = ctx.images(fw, download=False)
        route, info = _routes(ctx, len(cand))
        assert info["status"] == 0 and info["window_class"] == 0 and not (route & BIT_SHADOW_ANY).any()
        big = np.flatnonzero(route & BIT_SHADOW_BIG)
        assert len(big) > LGRID and ctx.fallbacks()["large_shadow_kernel_candidates"] == len(big), len(big)
        only = fw.copy()
        flat = only.reshape(-1)
        keep = np.zeros(len(flat), bool)
        keep[cand[big]] = True
        flat["valid"][~keep] = 0
        img, cand2 = ctx.images(only)
        route2, info2 = _routes(ctx, len(cand2))
        fb = ctx.fallbacks()
        assert info2["status"] == 0 and len(cand2) == len(big)
        assert fb["large_shadow_kernel_candidates"] > LGRID, fb
        assert fb["large_shadow_kernel_candidates"] == int(((route2 & BIT_SHADOW_BIG) != 0).sum())
        oimg, ocand = oracle_mod.images(p, xyz, nrm, cam, cl["view_points"], only)
        assert np.array_equal(cand2, ocand) and img.tobytes() == oimg.tobytes()
        print("large shadow kernel: %d, then %d candidates on %d workgroups" % (len(big), fb["large_shadow_kernel_candidates"], LGRID))
    finally:
        ctx.close()


def test_second_call_with_another_candidate_list(oracle_mod, small_cloud):
    """Two images() calls on one context: all candidates, then another list (every other one dropped, so that the hand
    sets keep other members and the workgroups other candidates) — the second result equals the oracle's for that list,
    and the first list once more gives the first bytes."""
    cl = small_cloud
    p = oracle_mod.default_params(15)
    si = synth.sample_indices(cl, 24)
    ctx = api.Context(api.default_params(15))
    try:
        ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
        img_a, cand_a, fw_a, route_a, info_a = _images(ctx, oracle_mod, p, cl["xyz"], cl["normals"], cl["cam_source"],
                                                       cl["view_points"], si)
        fw_b = fw_a.copy()
        flat = fw_b.reshape(-1)
        flat["valid"][np.flatnonzero(flat["valid"])[1::2]] = 0
        img_b, cand_b = ctx.images(fw_b)
        route_b, info_b = _routes(ctx, len(cand_b))
        oimg, ocand = oracle_mod.images(p, cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"], fw_b)
        assert 20 < len(cand_b) < len(cand_a)
        assert np.array_equal(cand_b, ocand) and img_b.tobytes() == oimg.tobytes()
        assert not route_b.any() and info_b["status"] == 0
        assert ctx.images_stats()["candidates"] == len(cand_b)
        img_c, cand_c = ctx.images(fw_a)
        assert np.array_equal(cand_c, cand_a) and img_c.tobytes() == img_a.tobytes()
    finally:
        ctx.close()
