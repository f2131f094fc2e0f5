"""gpd_hip_set_shadow_jitter on the device: the shadow channels (4, 9, 14 of 15) with every voxel's point moved by the seeded
draw of include/gpd_hip.h, byte for byte against the numpy restatement of tests/pyref_jitter.py — on every route of the image
stage the mode can take — and the properties of the setting: only the shadow moves, off is off, the stream of shadow draws is
untouched, and the images do not depend on the entry that made them.

The hand sets are supplied through images_given at lcg_base 0, the compared sets first, so the restatement draws the shadow of
those alone.  Each byte case first establishes on the restatement that its input decides something."""
import numpy as np
import pytest

import given_cases as gc
import pyref
import pyref_jitter as J
from gpd_amd import api, synth
from test_gpu_image_overflow_and_rays import _set_of
from test_gpu_image_paths import BIT_SHADOW_ANY, BIT_SHADOW_BIG, _dense_cloud, _pick

pytestmark = pytest.mark.gpu

SEED = 0x5EED5EED5EED
SHADOW = [4, 9, 14]
OTHERS = [c for c in range(15) if c not in SHADOW]
GPD_ERR_INVALID = -1


def _params(C=15, **over):
    p = api.default_params(C)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _context(p, cl, seed=SEED, on=True):
    ctx = api.Context(p)
    ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
    if on:
        ctx.set_shadow_jitter(True, seed)
    return ctx


def _radius(p):
    return max(p.volume_depth, p.volume_height / 2.0, p.volume_width)


def _box_aabb_range(p, hand):
    """[floor(min), floor(max)] per world axis of the voxel AABB of the hand's image box (shadow_image_body, jitter off)"""
    lo = np.array([hand["bottom"], hand["center"] - p.volume_width / 2.0, -p.volume_height])
    hi = np.array([hand["bottom"] + p.volume_depth, hand["center"] + p.volume_width / 2.0, p.volume_height])
    cs = np.array([[(hi if (c >> a) & 1 else lo)[a] for a in range(3)] for c in range(8)])
    w = np.asarray(hand["sample"], np.float64) + cs @ np.asarray(hand["frame"], np.float64).reshape(3, 3).T
    return np.floor(w.min(axis=0) * (1.0 / 0.003)), np.floor(w.max(axis=0) * (1.0 / 0.003))


def _restate(p, cl, hands, num_sets, seed, only=None, images=True):
    """The images of every candidate of the first `num_sets` live sets of `hands` [sets, slots] at lcg_base 0 ->
    ({candidate ordinal: image}, stats): stats counts, over those candidates, the voxels in a box only because they were moved,
    out of it only because they were moved, and in a box with a lattice position outside [floor(min), floor(max)] of the
    box's voxel AABB.  `only`: the candidate ordinals to restate (default: all of those sets); images False: the stats alone."""
    rng = pyref.Lcg(0)
    cam, vp = np.asarray(cl["cam_source"]).reshape(-1, len(cl["xyz"])), np.asarray(cl["view_points"], np.float64).reshape(-1, 3)
    want, stats, k, done = {}, dict(moved_in=0, moved_out=0, outside_aabb=0, in_box=0), 0, 0
    for s in range(hands.shape[0]):
        if not hands[s]["valid"].any():
            continue
        if done == num_sets:
            break
        nbr = pyref.radius_neighbours(cl["xyz"], hands[s, 0]["sample"].astype(np.float32), _radius(p))
        if cam.shape[0] == 1:
            vox = J.shadow_voxels(cl["xyz"][nbr], vp[0], rng, _radius(p))
        else:
            vox = J.shadow_voxels_cameras(cl["xyz"][nbr], cam[:, nbr], vp, rng, _radius(p))
        va = np.asarray(vox, np.int64).reshape(-1, 3)
        for j in range(hands.shape[1]):
            if not hands[s, j]["valid"]:
                continue
            h = hands[s, j]
            if only is not None and k not in only:
                k += 1
                continue
            want[k] = J.grasp_image_jitter(p, h, cl["xyz"], cl["normals"], nbr, vox, seed) if images else None
            a, b = J.in_box(p, h, J.lattice_points(va)), J.in_box(p, h, J.shadow_points(va, seed))
            f0, f1 = _box_aabb_range(p, h)
            stats["moved_in"] += int((b & ~a).sum())
            stats["moved_out"] += int((a & ~b).sum())
            stats["in_box"] += int(b.sum())
            stats["outside_aabb"] += int((b & ((va < f0) | (va > f1)).any(axis=1)).sum())
            k += 1
        done += 1
    assert done == num_sets
    return want, stats


def _assert_bytes(img, want, what):
    assert len(want) > 0
    for k, w in want.items():
        bad = [c for c in range(15) if not np.array_equal(img[k][..., c], w[..., c])]
        assert not bad, (what, "candidate %d: channels %s differ, %d pixels" % (k, bad, int((img[k] != w).sum())))


@pytest.fixture(scope="module")
def scene():
    """6000 points, one camera at the origin, and the records a search returns for six samples"""
    cl, si = gc.scene(two_cameras=False)
    si = si[:6]
    ctx = api.Context(api.default_params(15))
    try:
        ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
        hands = ctx.search(si)
    finally:
        ctx.close()
    assert (hands["valid"].astype(bool).any(axis=1)).sum() >= 3
    hands.setflags(write=False)
    return cl, si, hands


# ---- 1. bytes, and 4a: the wide instantiation -----------------------------------------------------------------------------
def test_bytes_one_camera_stock_geometry_on_the_wide_windows(scene):
    cl, si, hands = scene
    p = _params()
    want, stats = _restate(p, cl, hands, 2, SEED)
    print("stock geometry:", stats, "over", len(want), "candidates")
    assert stats["moved_in"] >= 1 and stats["moved_out"] >= 1, stats
    ctx = _context(p, cl)
    try:
        img, cand, draws = ctx.images_given(hands)
        route, info = ctx.image_routes()
        assert info["status"] == 0 and info["window_class"] == 1 and info["set_mode"] == 1, info
        assert not (route & (BIT_SHADOW_BIG | BIT_SHADOW_ANY)).any()  # shadow_image_kernel<SH_CAP, WIDE, JIT> alone
        _assert_bytes(img, want, "stock geometry")
        assert all((img[k][..., SHADOW] > 0).any() for k in want)
    finally:
        ctx.close()


# ---- 2. the widened window: boxes whose faces are parallel to the lattice ----------------------------------------------------
def _lattice_sets(scene, p):
    """-> ([2, slots] hand sets at one sample, stats of the first): the identity frame in every slot (different bottoms and
    centers), then the same turned 45 degrees about z.  The sample is the first of the scene's whose identity set gains voxels
    from outside the voxel AABB of a box: those lie outside the window floor(min) - 1 .. floor(max) + 1 minus its margins."""
    cl, si, hands = scene
    slots = hands.shape[1]
    bottoms = np.linspace(-0.045, 0.0, slots)
    centers = np.linspace(-0.05, 0.05, slots)
    x64 = cl["xyz"].astype(np.float64)
    for s in range(len(si)):
        smp = x64[si[s]]
        a = _set_of(hands[s], smp, [np.eye(3)] * slots, 0.0, centers)
        for j in range(slots):
            a[0, j]["bottom"] = bottoms[j]
        Rz = gc._rotation(np.array([0.0, 0.0, 1.0]), np.pi / 4)
        b = _set_of(hands[s], smp, [Rz] * slots, -0.02, centers[::-1])
        f = np.ascontiguousarray(np.concatenate([a, b]))
        _, stats = _restate(p, cl, f, 1, SEED, images=False)
        if stats["outside_aabb"] >= 1 and stats["moved_in"] >= 1 and stats["moved_out"] >= 1:
            return f
    raise AssertionError("no sample of the scene gains a voxel from outside a box's voxel AABB")


def test_boxes_parallel_to_the_lattice_gain_voxels_from_outside_the_old_window(scene):
    cl, si, hands = scene
    p = _params()
    f = _lattice_sets(scene, p)
    assert api.given_check(p, f) is None
    want, stats = _restate(p, cl, f, 2, SEED)
    print("lattice-parallel boxes:", stats, "over", len(want), "candidates")
    assert len(want) == 2 * hands.shape[1] and stats["outside_aabb"] >= 1, stats
    ctx = _context(p, cl)
    try:
        img, cand, draws = ctx.images_given(f)
        assert ctx.image_routes()[1]["status"] == 0
        _assert_bytes(img, want, "lattice-parallel boxes")
    finally:
        ctx.close()


# ---- 3. two cameras -----------------------------------------------------------------------------------------------------------
def test_two_cameras_intersect_on_voxels_then_move():
    cl, si = gc.scene(two_cameras=True)
    p = _params()
    ctx = _context(p, cl)
    try:
        hands = ctx.search(si[:3])
        want, stats = _restate(p, cl, hands, 1, SEED)
        print("two cameras:", stats, "over", len(want), "candidates")
        assert stats["in_box"] >= 1 and stats["moved_in"] + stats["moved_out"] >= 1, stats
        img, cand, draws = ctx.images_given(hands)
        assert ctx.image_routes()[1]["status"] == 0
        _assert_bytes(img, want, "two cameras")
        # the intersection is not the first camera's set: one camera alone gives other shadow planes
        one = dict(cl, cam_source=np.ascontiguousarray(cl["cam_source"][:1]), view_points=np.ascontiguousarray(cl["view_points"][:1]))
        ctx.upload_cloud(one["xyz"], one["normals"], one["cam_source"], one["view_points"])
        img1, _, _ = ctx.images_given(hands)
        ks = sorted(want)
        assert img1[ks][..., SHADOW].tobytes() != img[ks][..., SHADOW].tobytes()
        assert img1[ks][..., OTHERS].tobytes() == img[ks][..., OTHERS].tobytes()
    finally:
        ctx.close()


# ---- 4. the other routes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,over,window_class", [
    ("huge_image_volume", dict(volume_width=0.16, volume_depth=0.10), 2),  # shadow_set_kernel<2>, shadow_image_any_kernel<JIT>
    ("small_image_volume", dict(volume_width=0.08, volume_depth=0.05), 0),  # shadow_set_kernel<0, JIT>, the 46^3 windows
])
def test_bytes_on_the_general_kernel_and_on_the_default_windows(name, over, window_class):
    cl = synth.make_cloud(4242, 8000)
    si = synth.sample_indices(cl, 4)
    p = _params(**over)
    assert api.image_model(p, 1)["window_class"] == window_class
    ctx = _context(p, cl)
    try:
        hands = ctx.search(si)
        want, stats = _restate(p, cl, hands, 1, SEED)
        print(name, stats, "over", len(want), "candidates")
        assert stats["moved_in"] >= 1 and stats["moved_out"] >= 1, stats
        # twice: the default windows' set kernel writes only the rows its candidates can see, the second launch finds the first's bits
        for _ in range(2):
            img, cand, draws = ctx.images_given(hands)
            route, info = ctx.image_routes()
            assert info["status"] == 0 and info["window_class"] == window_class == info["set_mode"], info
            assert not (route & (BIT_SHADOW_BIG | BIT_SHADOW_ANY)).any()
            _assert_bytes(img, want, name)
    finally:
        ctx.close()


def test_bytes_on_the_large_capacity_instantiation():
    """Under a locally eleven-fold surface a box holds more shadow voxels than shadow_image_kernel<SH_CAP> lists: the wide,
    jittered large instantiation redoes it.  A search's candidates show which set has such a box; that set is compared."""
    p = _params()
    cl0, xyz, nrm, cam, near, far = _dense_cloud(10, 0.1)
    cl = dict(xyz=xyz, normals=nrm, cam_source=cam, view_points=cl0["view_points"])
    ctx = _context(p, cl)
    try:
        hands = ctx.search(_pick(near, 24, 9))
        _, cand = ctx.images_given(hands, download=False)[:2]
        route, info = ctx.image_routes()
        assert info["status"] == 0 and info["window_class"] == 1
        big = np.flatnonzero(route & BIT_SHADOW_BIG)
        assert 0 < len(big) < len(route), (len(big), len(route))
        s = int(cand[big[0]]) // hands.shape[1]
        one = np.ascontiguousarray(hands[s:s + 1])
        _, c1 = ctx.images_given(one, download=False)[:2]
        r1 = ctx.image_routes()[0]
        assert (r1 & BIT_SHADOW_BIG).any()
        # the queued candidates (two at the most) and one that was not (the restatement is per point, in Python)
        only = set(np.flatnonzero(r1 & BIT_SHADOW_BIG)[:2].tolist()) | set(np.flatnonzero((r1 & BIT_SHADOW_BIG) == 0)[:1].tolist())
        want, stats = _restate(p, cl, one, 1, SEED, only)
        print("large instantiation:", stats, "over", len(want), "candidates,", len(big), "of", len(route), "queued")
        img, c1, _ = ctx.images_given(one)
        r1, i1 = ctx.image_routes()
        assert i1["status"] == 0 and (r1 & BIT_SHADOW_BIG).any() and not (r1 & BIT_SHADOW_ANY).any()
        _assert_bytes(img, want, "large instantiation")
    finally:
        ctx.close()


# ---- 5. only the shadow moves; 6. off is off -----------------------------------------------------------------------------------
def test_only_the_shadow_channels_depend_on_the_setting_and_the_seed(scene):
    cl, si, hands = scene
    p = _params()
    ctx = _context(p, cl, on=False)
    never = _context(p, cl, on=False)
    try:
        off, cand0, d0 = ctx.images_given(hands)
        assert ctx.image_routes()[1]["window_class"] == 0
        ctx.set_shadow_jitter(True, SEED)
        on, cand1, d1 = ctx.images_given(hands)
        assert ctx.image_routes()[1]["window_class"] == 1
        ctx.set_shadow_jitter(True, SEED + 1)
        on2, cand2, d2 = ctx.images_given(hands)
        assert d0 == d1 == d2 > 0 and np.array_equal(cand0, cand1) and np.array_equal(cand0, cand2)
        assert off[..., OTHERS].tobytes() == on[..., OTHERS].tobytes() == on2[..., OTHERS].tobytes()
        for c in SHADOW:
            assert off[..., c].tobytes() != on[..., c].tobytes() and on[..., c].tobytes() != on2[..., c].tobytes(), c
        # the same seed again: the same bytes; then off: the bytes of a context that never had it on
        ctx.set_shadow_jitter(True, SEED)
        assert ctx.images_given(hands)[0].tobytes() == on.tobytes()
        ctx.set_shadow_jitter(False)
        back, _, d3 = ctx.images_given(hands)
        assert ctx.image_routes()[1]["window_class"] == 0 and d3 == d0
        ref, _, _ = never.images_given(hands)
        assert back.tobytes() == off.tobytes() == ref.tobytes()
    finally:
        ctx.close()
        never.close()


@pytest.mark.parametrize("C", [12, 3])
def test_without_a_shadow_channel_the_setting_changes_nothing(scene, C):
    cl, si, _ = scene
    ctx = _context(_params(C), cl, on=False)
    try:
        hands = ctx.search(si)
        off, _, d0 = ctx.images_given(hands)
        ctx.set_shadow_jitter(True, SEED)
        on, _, d1 = ctx.images_given(hands)
        assert ctx.image_routes()[1]["window_class"] == 0
        assert off.shape[-1] == C and len(off) > 0 and on.tobytes() == off.tobytes() and d0 == d1
    finally:
        ctx.close()


def test_setter_refusals(scene):
    cl, si, hands = scene
    ctx = _context(_params(), cl)
    try:
        want = ctx.images_given(hands)[0]
        for bad in (2, -1, 256):
            assert api.lib().gpd_hip_set_shadow_jitter(ctx._h, bad, 1) == GPD_ERR_INVALID
        assert ctx.images_given(hands)[0].tobytes() == want.tobytes()  # ... and changed nothing
    finally:
        ctx.close()


# ---- 7. the images do not depend on the entry ----------------------------------------------------------------------------------
def test_images_after_a_search_and_replay_equal_images_given(scene, lenet15_real):
    cl, si, _ = scene
    ctx = _context(_params(), cl)
    try:
        ctx.set_lenet_weights(lenet15_real)
        hands = ctx.search(si)
        a, ca = ctx.images(hands)
        # a resident list is re-launched under the setting in force: replay after a switch scores the other images
        ctx.replay(3)
        s_on = ctx.replay_times(len(ca))[3]
        ctx.set_shadow_jitter(False)
        ctx.replay(3)
        s_off = ctx.replay_times(len(ca))[3]
        ctx.set_shadow_jitter(True, SEED)
        ctx.replay(3)
        assert ctx.replay_times(len(ca))[3].tobytes() == s_on.tobytes() != s_off.tobytes()
        b, cb, _ = ctx.images_given(hands)
        assert np.array_equal(ca, cb) and len(ca) > 0 and a.tobytes() == b.tobytes()
        assert ctx.score(b).tobytes() == s_on.tobytes()
        ctx.set_shadow_jitter(False)
        assert ctx.score(ctx.images_given(hands)[0]).tobytes() == s_off.tobytes()
    finally:
        ctx.close()


def test_batch_and_sharded_equal_the_single_call(lenet15_real):
    cl_a = synth.make_cloud(4242, 8000)
    cl_b = synth.make_cloud(77, 6000)
    si_a, si_b = synth.sample_indices(cl_a, 10), synth.sample_indices(cl_b, 8)
    p = _params()
    ctx, other = _context(p, cl_a), _context(p, cl_a)
    try:
        for c in (ctx, other):
            c.set_lenet_weights(lenet15_real)
            c.set_lenet_mode(api.LENET_F32_CHAIN)
        single = []
        for cl, s in ((cl_a, si_a), (cl_b, si_b)):
            ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
            h, ns, nc = ctx.detect_select(s)
            single.append((h.copy(), ns, nc))
        assert single[0][2] > 0 and single[1][2] > 0
        got = ctx.detect_batch([cl_a, cl_b], [si_a, si_b])
        for g, w in zip(got, single):
            assert (g[1], g[2]) == (w[1], w[2]) and g[0].tobytes() == w[0].tobytes()
        sh, info = ctx.detect_sharded([other], cl_a, si_a, [4])
        assert sum(i[1] for i in info) == single[0][2] and info[1][2] == info[0][3]
        assert sh.tobytes() == single[0][0].tobytes()
        # the setting is each context's own: the other context off gives other scores for its range
        other.set_shadow_jitter(False)
        sh2, _ = ctx.detect_sharded([other], cl_a, si_a, [4])
        n0 = info[0][1]
        assert sh2[:n0].tobytes() == sh[:n0].tobytes() and sh2[n0:]["score"].tobytes() != sh[n0:]["score"].tobytes()
        # and with it off everywhere the scores are those of a jitter-free single call
        ctx.set_shadow_jitter(False)
        ctx.upload_cloud(cl_a["xyz"], cl_a["normals"], cl_a["cam_source"], cl_a["view_points"])
        assert ctx.detect_select(si_a)[0]["score"].tobytes() != single[0][0]["score"].tobytes()
    finally:
        ctx.close()
        other.close()


def test_label_view_returns_the_images_of_images_given(oracle_mod):
    """The view of tests/entry_cases.py on the default variant (its rounds, its ground truth), all four rounds: every
    round's candidate list is imaged from the start of the stream of draws, as images_given images it at lcg_base 0."""
    import entry_cases as ec
    import ref_cases as rc
    cl = rc.cloud("default_c15")
    gt, gn = ec.ground_truth("default_c15")
    rounds = ec.view_rounds("default_c15")
    p = _params()
    ctx = _context(p, cl)
    try:
        ctx.upload_ground_truth(gt, gn)
        view = ctx.label_view(rounds, ec.MIN_POSITIVES, ec.MAX_GRASPS_PER_VIEW)
        print("label_view: %d candidates, %d positives, %d kept" % (view["num_candidates"], view["num_positives"], view["num_out"]))
        assert view["rounds_run"] == len(rounds) and view["num_out"] > 0
        imgs = []
        for r in range(len(rounds)):
            fw = oracle_mod.filter_workspace(oracle_mod.default_params(15), ctx.search(rounds[r]).copy())
            imgs.append(ctx.images_given(fw)[0])
        allimg = np.concatenate(imgs)
        assert len(allimg) == view["num_candidates"]
        assert view["images"].tobytes() == allimg[view["src_index"]].tobytes()
        ctx.set_shadow_jitter(False)
        off = ctx.label_view(rounds, ec.MIN_POSITIVES, ec.MAX_GRASPS_PER_VIEW)
        assert np.array_equal(off["src_index"], view["src_index"]) and np.array_equal(off["labels"], view["labels"])
        assert off["images"][..., OTHERS].tobytes() == view["images"][..., OTHERS].tobytes()
        assert off["images"][..., SHADOW].tobytes() != view["images"][..., SHADOW].tobytes()
    finally:
        ctx.close()
