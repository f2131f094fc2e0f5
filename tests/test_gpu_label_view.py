"""gpd_hip_label_view (one view of DataGenerator::generateData on the device) and the resident ground-truth slot against the
oracle's own entries composed per round (tests/label_view_cases.py): search -> filter_workspace -> images for the candidates,
reevaluate on the ground truth for labels and flags, balanceInstances restated in Python.  Every comparison is byte for byte:
images, labels, the whole record array, src_index, all_labels, round_counts."""
import ctypes as C

import numpy as np
import pytest

import label_view_cases as lvc
import ref_cases as rcs
from gpd_amd import api, synth
from test_gpu_reevaluate import _dense

pytestmark = pytest.mark.gpu

GT_SEED, ROUNDS_SEED, SAMPLES_PER_ROUND = 7, 7, 16
HAND_BYTES = api.HAND_DTYPE.itemsize


def _rounds(cl, rounds, seed=ROUNDS_SEED, per=SAMPLES_PER_ROUND):
    rng = np.random.RandomState(seed)
    obj = np.flatnonzero(cl["is_object"])
    return np.stack([rng.choice(obj, per, replace=False) for _ in range(rounds)]).astype(np.int32)


def _case(name, default_params, **over):
    """(params, cloud, cam, vp) of a variant of tests/ref_cases.py, with further parameter overrides."""
    p, cl, _, cam, vp = rcs.case_inputs(name, default_params)
    return rcs.set_params(p, **over), cl, cam, vp


_want = {}


def _expected(om, name, over, rounds, min_positives, max_grasps):
    """The oracle's view of a case: computed once per (case, settings), shared by the tests, never modified."""
    key = (name, tuple(sorted((k, str(v)) for k, v in over.items())), rounds.tobytes(), min_positives, max_grasps)
    if key not in _want:
        op, cl, cam, vp = _case(name, om.default_params, **over)
        gt, gn, _ = rcs.ground_truth(cl["xyz"], cl["normals"], GT_SEED)
        _want[key] = lvc.expected_view(om, op, cl["xyz"], cl["normals"], cam, vp, gt, gn, rounds, min_positives, max_grasps)
    return _want[key]


def _context(name, **over):
    gp, cl, cam, vp = _case(name, api.default_params, **over)
    ctx = api.Context(gp)
    gt, gn, _ = rcs.ground_truth(cl["xyz"], cl["normals"], GT_SEED)
    ctx.upload_ground_truth(gt, gn)
    ctx.upload_cloud(cl["xyz"], cl["normals"], cam, vp)
    return ctx, cl


def _d2h_bound(got, channels, all_labels):
    return got["num_out"] * (3600 * channels + HAND_BYTES + 5) + all_labels + 64 * got["rounds_run"] + 4096


# ---- 1. the base case ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_grasps, num_out", [(4, 4), (5, 4), (500, 6)])
def test_base_case(oracle_mod, max_grasps, num_out):
    rounds = _rounds(rcs.cloud(), 6)
    want = _expected(oracle_mod, "default_c15", {}, rounds, 3, max_grasps)
    # the numbers the issue states for this case
    assert want["round_counts"].tolist() == [[24, 0], [43, 1], [30, 1], [31, 1], [0, 0], [0, 0]]
    assert (want["rounds_run"], want["num_candidates"], want["num_positives"], want["num_out"]) == (4, 128, 3, num_out)
    # in rounds 0 and 2 the ground truth disagrees with the search's own flags: the labels are not a copy of them
    edges = np.concatenate([[0], np.cumsum(want["round_counts"][:, 0])])
    differ = [bool((want["search_flags"][a:b] != want["all_labels"][a:b]).any()) for a, b in zip(edges[:4], edges[1:5])]
    assert differ[0] and differ[2], differ
    ctx, _ = _context("default_c15")
    try:
        got = ctx.label_view(rounds, 3, max_grasps, want_all_labels=True)
        lvc.assert_view(got, want, "max_grasps_per_view=%d" % max_grasps)
        # round 0 has no positive and later rounds have: every kept image is the image of its own record
        assert got["images"].tobytes() == want["all_images"][got["src_index"]].tobytes()
        assert got["hands"].tobytes() == want["all_hands"][got["src_index"]].tobytes()
        assert (got["src_index"][: got["num_positives_out"]] >= 24).all() and (got["src_index"][got["num_positives_out"]:] < 24).all()
        # 2. what was built and what crossed PCIe
        assert got["gt_neighbourhoods"] == sum(want["sets_with_candidates"]) < got["num_candidates"]
        assert 0 < got["d2h_bytes"] <= _d2h_bound(got, 15, got["num_candidates"]), got["d2h_bytes"]
        print("label_view: %d rounds, %d candidates, %d positives, %d kept, %d lists, %d bytes to the host, stage ms %s"
              % (got["rounds_run"], got["num_candidates"], got["num_positives"], got["num_out"], got["gt_neighbourhoods"], got["d2h_bytes"],
                 ["%.3f" % m for m in got["stage_ms"]]))
    finally:
        ctx.close()


@pytest.mark.parametrize("name, over", [("default_c3", {}), ("two_cameras", {}), ("offlattice_c15", {}),
                                        ("default_c15", dict(hand_axes=[0, 1, 2]))],
                         ids=["c3", "two_cameras", "offlattice_c15", "three_axes"])
def test_other_cases(oracle_mod, name, over):
    rounds = _rounds(rcs.cloud(name), 6)
    want = _expected(oracle_mod, name, over, rounds, 3, 500)
    assert want["num_candidates"] > 0 and want["num_positives"] > 0
    ctx, _ = _context(name, **over)
    try:
        got = ctx.label_view(rounds, 3, 500, want_all_labels=True)
        lvc.assert_view(got, want, name)
        assert got["gt_neighbourhoods"] == sum(want["sets_with_candidates"]) < got["num_candidates"]
        assert got["d2h_bytes"] <= _d2h_bound(got, ctx.params.image_num_channels, got["num_candidates"]), got["d2h_bytes"]
        no_all = ctx.label_view(rounds, 3, 500)
        assert "all_labels" not in no_all and no_all["d2h_bytes"] <= _d2h_bound(no_all, ctx.params.image_num_channels, 0)
        lvc.assert_view(no_all, want, name + " without all_labels")
    finally:
        ctx.close()


# ---- 3. persistence --------------------------------------------------------------------------------------------------------
def test_ground_truth_stays_across_other_calls(oracle_mod, lenet15_real):
    om = oracle_mod
    op = om.default_params(15)
    cl = rcs.cloud()
    gt, gn, _ = rcs.ground_truth(cl["xyz"], cl["normals"], GT_SEED)
    rounds = _rounds(cl, 6)
    half = {k: np.ascontiguousarray(cl[k][::2]) for k in ("xyz", "normals")}
    half_cam = np.ascontiguousarray(cl["cam_source"][:, ::2])
    half_rounds = np.stack([np.random.RandomState(3 + r).choice(len(half["xyz"]), 16, replace=False) for r in range(4)]).astype(np.int32)
    si = synth.sample_indices(cl, 24)
    ctx = api.Context(api.default_params(15))
    try:
        ctx.set_lenet_weights(lenet15_real)
        ctx.upload_ground_truth(gt, gn)  # once
        ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
        lvc.assert_view(ctx.label_view(rounds, 3, 500, want_all_labels=True), _expected(om, "default_c15", {}, rounds, 3, 500), "the scene")
        hands, n_cand = ctx.detect(si)  # a detect and an upload in between
        ctx.upload_cloud(half["xyz"], half["normals"], half_cam, cl["view_points"])
        want = lvc.expected_view(om, op, half["xyz"], half["normals"], half_cam, cl["view_points"], gt, gn, half_rounds, 1000, 500)
        assert want["num_candidates"] > 0
        lvc.assert_view(ctx.label_view(half_rounds, 1000, 500, want_all_labels=True), want, "every second point")
        # the view slot and the search buffers are the other entries' again: reevaluate on the uploaded cloud, then a detect
        recs = want["all_hands"][:64]
        labels, out = ctx.reevaluate(recs)
        wl, wout = om.reevaluate(op, half["xyz"], half["normals"], recs)
        assert np.array_equal(labels, wl) and out.tobytes() == wout.tobytes()
        ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
        ctx.label_view(rounds, 3, 4)
        hands, n_cand = ctx.detect(si)
        ohands, on_cand, _ = om.detect(op, cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"], si, lenet15_real)
        assert n_cand == on_cand and n_cand > 0
        a, b = hands.copy(), ohands.copy()
        assert np.abs(a["score"] - b["score"]).max() <= 1e-4
        a["score"] = 0
        b["score"] = 0
        assert a.tobytes() == b.tobytes()
    finally:
        ctx.close()


# ---- 4. ground-truth list tiers --------------------------------------------------------------------------------------------
def test_ground_truth_lists_beyond_the_lds_capacities(oracle_mod, cloud30k):
    om, cl = oracle_mod, cloud30k
    op = om.default_params(15)
    gt, gn = _dense(cl, 3)  # 120k points: neighbourhoods of up to 25k, beyond the 16384-entry lists
    rounds = synth.sample_indices(cl, 125, seed=31).reshape(1, -1)
    want = lvc.expected_view(om, op, cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"], gt, gn, rounds, 10 ** 6, 500)
    assert 0 < want["num_positives"] < want["num_candidates"]
    # the hand neighbourhoods (0.11 m: outer diameter - finger width) of the sets' samples do not fit the LDS lists
    samples = np.unique(want["all_hands"]["sample"], axis=0)
    assert max(len(om.radius_search(gt, s.astype(np.float32), 0.11)[0]) for s in samples[::8]) > 16384
    ctx = api.Context(api.default_params(15))
    try:
        ctx.upload_ground_truth(gt, gn)
        ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
        got = ctx.label_view(rounds, 10 ** 6, 500, want_all_labels=True)
        lvc.assert_view(got, want, "dense ground truth")
        assert got["all_labels"].any() and not got["all_labels"].all()
        assert got["gt_neighbourhoods"] == sum(want["sets_with_candidates"]) < got["num_candidates"]
        assert got["d2h_bytes"] <= _d2h_bound(got, 15, got["num_candidates"])
    finally:
        ctx.close()


def test_ground_truth_list_retry_to_16384_entries(oracle_mod):
    """The round's list-capacity retry 8192 -> 16384 entries (the in-place bitonic sort), which the dense ground truth above jumps
    over: a ground truth of 1000 scattered points plus 9000 jittered copies of the points within 5 cm of one of the round's four
    samples, so that sample's list holds more than 8192 and fewer than 16384 points.  Then a sparse ground truth on the same
    context.  Both views byte for byte against the oracle."""
    om = oracle_mod
    op = om.default_params(15)
    cl = rcs.cloud()
    xyz, nrm = cl["xyz"], cl["normals"]
    rounds = _rounds(cl, 6)[2:3, 12:]  # four samples: two hand sets with candidates
    sparse = np.arange(0, len(xyz), 8)
    ball = np.flatnonzero(np.linalg.norm(xyz - xyz[rounds[0, 3]], axis=1) < 0.05)
    rng = np.random.RandomState(11)
    idx = ball[rng.randint(0, len(ball), 9000)]
    dense_xyz = np.concatenate([xyz[sparse], (xyz[idx] + rng.uniform(-0.0003, 0.0003, (9000, 3))).astype(np.float32)])
    dense_nrm = np.concatenate([nrm[sparse], nrm[idx]])
    ctx = api.Context(api.default_params(15))
    try:
        ctx.upload_cloud(xyz, nrm, cl["cam_source"], cl["view_points"])
        for what, gt, gn in (("dense cluster", dense_xyz, dense_nrm), ("sparse", xyz[sparse].copy(), nrm[sparse].copy())):
            want = lvc.expected_view(om, op, xyz, nrm, cl["cam_source"], cl["view_points"], gt, gn, rounds, 10 ** 6, 500)
            assert want["num_candidates"] == 9
            sizes = [len(om.radius_search(gt, s.astype(np.float32), 0.11)[0]) for s in np.unique(want["all_hands"]["sample"], axis=0)]
            if what == "sparse":
                assert max(sizes) < 8192 and want["num_positives"] == 0
            else:  # the cluster decides a label: without it the view has no positive
                assert 8192 < max(sizes) < 16384 and min(sizes) < 8192 and want["num_positives"] == 1, sizes
            ctx.upload_ground_truth(gt, gn)
            got = ctx.label_view(rounds, 10 ** 6, 500, want_all_labels=True)
            lvc.assert_view(got, want, what)
            assert got["gt_neighbourhoods"] == 2
    finally:
        ctx.close()


# ---- 5. edges --------------------------------------------------------------------------------------------------------------
def _raw_job(ctx, rounds, min_positives, max_grasps, capacity):
    j = api.LabelViewJob()
    keep = dict(sr=np.ascontiguousarray(rounds, np.int32), img=np.full((max(capacity, 1), 60, 60, ctx.params.image_num_channels), 7, np.uint8),
                lab=np.full(max(capacity, 1), 7, np.uint8))
    j.sample_indices, j.max_rounds, j.samples_per_round = api._ptr(keep["sr"]), keep["sr"].shape[0], keep["sr"].shape[1]
    j.min_positives, j.max_grasps_per_view = min_positives, max_grasps
    j.images, j.labels, j.capacity = api._ptr(keep["img"]), api._ptr(keep["lab"]), capacity
    return j, keep


def test_edges(oracle_mod):
    om = oracle_mod
    cl = rcs.cloud()
    rounds = _rounds(cl, 6)
    gt, gn, _ = rcs.ground_truth(cl["xyz"], cl["normals"], GT_SEED)
    ctx = api.Context(api.default_params(15))
    try:
        ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
        # no ground truth: GPD_ERR_STATE; also after it was cleared
        j, keep = _raw_job(ctx, rounds, 3, 4, 4)
        assert api.lib().gpd_hip_label_view(ctx._h, C.byref(j)) == -4
        ctx.upload_ground_truth(gt, gn)
        ctx.upload_ground_truth(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
        assert api.lib().gpd_hip_label_view(ctx._h, C.byref(j)) == -4
        ctx.upload_ground_truth(gt, gn)
        # a capacity below 2 * floor(max / 2): GPD_ERR_INVALID, nothing written
        for max_grasps, capacity in ((4, 3), (5, 3), (500, 6)):
            j, keep = _raw_job(ctx, rounds, 3, max_grasps, capacity)
            assert api.lib().gpd_hip_label_view(ctx._h, C.byref(j)) == -1
            assert (keep["img"] == 7).all() and (keep["lab"] == 7).all() and j.rounds_run == 0 and j.num_out == 0 and j.d2h_bytes == 0
        j, keep = _raw_job(ctx, rounds, 3, 5, 4)  # 2 * floor(5 / 2) is enough
        assert api.lib().gpd_hip_label_view(ctx._h, C.byref(j)) == 0 and j.num_out == 4
        # min_positives = 0 runs no round
        got = ctx.label_view(rounds, 0, 500, want_all_labels=True)
        assert (got["rounds_run"], got["num_candidates"], got["num_out"], got["gt_neighbourhoods"]) == (0, 0, 0, 0)
        assert len(got["all_labels"]) == 0 and not got["round_counts"].any()
    finally:
        ctx.close()
    # a workspace that filters every hand: all rounds run, nothing found, status OK
    gp = rcs.set_params(api.default_params(15), workspace_grasps=[5.0, 6.0, 5.0, 6.0, 5.0, 6.0])
    ctx = api.Context(gp)
    try:
        ctx.upload_ground_truth(gt, gn)
        ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
        got = ctx.label_view(rounds, 3, 500, want_all_labels=True)
        assert (got["num_candidates"], got["rounds_run"], got["num_out"], got["num_positives"]) == (0, len(rounds), 0, 0)
        assert got["images"].shape == (0, 60, 60, 15) and not got["round_counts"].any()
    finally:
        ctx.close()


def test_unreachable_min_positives_runs_every_round(oracle_mod):
    rounds = _rounds(rcs.cloud(), 12, seed=19)
    want = _expected(oracle_mod, "default_c15", {}, rounds, 10 ** 6, 500)
    assert want["rounds_run"] == 12 and want["num_candidates"] > 3 * want["round_counts"][0, 0] > 0  # the accumulator has to grow
    ctx, _ = _context("default_c15")
    try:
        got = ctx.label_view(rounds, 10 ** 6, 500, want_all_labels=True)
        lvc.assert_view(got, want, "12 rounds")
        assert got["num_out"] == 2 * min(want["num_positives"], want["num_candidates"] - want["num_positives"])
        assert got["d2h_bytes"] <= _d2h_bound(got, 15, got["num_candidates"])
        lvc.assert_view(ctx.label_view(rounds, 10 ** 6, 500, want_all_labels=True), want, "12 rounds, again")
    finally:
        ctx.close()
