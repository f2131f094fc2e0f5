"""HandSearch::reevaluateHypotheses on the device (reeval_kernel, hand_search.cpp:66-134, 190-228) as widely as the search is
checked: every parameter variant of tests/ref_cases.py that changes the hand or the search, on the hands' own cloud and on a
"ground truth" made from it; ground-truth clouds whose neighbourhoods need the 16384-entry bitonic lists and the global-memory
lists; the edges of the label path; and an independent numpy restatement (tests/pyref_hands.reevaluate).

Every call is compared with oracle.reevaluate byte for byte (labels, the whole returned record array, the half and full
flags), and every call with more than one hand must see some labels 1 and some 0, except on normals estimated on the device,
where some variants have no full grasp left (there it must see label 0 and half flags)."""
import numpy as np
import pytest

import pyref_hands
import ref_cases as rcs
from gpd_amd import api, synth

pytestmark = pytest.mark.gpu

# variants that change the hand or the search parameters (the camera-only and channel-only ones do not reach this path)
VARIANTS = [n for n, (_, over, _) in rcs.VARIANTS.items() if over or n.startswith("offlattice")]
# the small hand closes on no object of the 8000-point scene as a full antipodal grasp; the 30k scene has a few
OTHER_SCENE = {"small_hand": (1234, 30000, 600)}
EXTRA_SAMPLES = 96


def check(ctx, op, xyz, normals, hands, mixed=True):
    """ctx.reevaluate(hands) against oracle.reevaluate on the uploaded cloud (xyz, normals) -> (labels, records)."""
    import oracle
    labels, out = ctx.reevaluate(hands)
    wl, wout = oracle.reevaluate(op, xyz, normals, hands)
    assert labels.dtype == np.int32 and labels.shape == (len(hands),)
    assert np.array_equal(labels, wl), np.flatnonzero(labels != wl)[:20]
    assert np.array_equal(out["half_antipodal"], wout["half_antipodal"])
    assert np.array_equal(out["full_antipodal"], wout["full_antipodal"])
    assert out.tobytes() == wout.tobytes()
    assert np.array_equal(out["full_antipodal"].astype(np.int32), labels)
    if mixed:
        assert 0 < int(labels.sum()) < len(labels), (int(labels.sum()), len(labels))
    print("reevaluate: %d hands, %d label 1, %d label 0, list capacity %d" % (len(labels), int(labels.sum()),
                                                                          int((labels == 0).sum()), ctx.fallbacks()["neighbourhood_list_capacity"]))
    return labels, out


def _variant_inputs(name, default_params):
    p, cl, si, cam, vp = rcs.case_inputs(name, default_params)
    if name in OTHER_SCENE:
        seed, P, S = OTHER_SCENE[name]
        cl = synth.make_cloud(seed, P)
        return p, cl, synth.sample_indices(cl, S), cl["cam_source"], cl["view_points"]
    obj = np.flatnonzero(cl["is_object"])
    extra = np.random.RandomState(11).choice(obj, EXTRA_SAMPLES, replace=False).astype(np.int32)
    return p, cl, np.concatenate([si, extra]), cam, vp


@pytest.mark.parametrize("name", VARIANTS)
def test_variant_same_cloud_and_ground_truth(oracle_mod, name):
    gp, cl, si, cam, vp = _variant_inputs(name, api.default_params)
    op = _variant_inputs(name, oracle_mod.default_params)[0]
    ctx = api.Context(gp)
    try:
        ctx.upload_cloud(cl["xyz"], cl["normals"], cam, vp)
        hands = ctx.search(si).reshape(-1)
        assert hands.tobytes() == oracle_mod.search(op, cl["xyz"], cl["normals"], si).reshape(-1).tobytes()
        # (a) the same cloud: valid and invalid records alike; the labels of the valid ones are the search's own flags
        labels, _ = check(ctx, op, cl["xyz"], cl["normals"], hands)
        v = hands["valid"].astype(bool)
        assert np.array_equal(labels[v], hands["full_antipodal"][v].astype(np.int32))
        # (b) a ground truth made from it: seeded subsample, sub-millimetre jitter; first with the kept points' normals ...
        gt, gn, sel = rcs.ground_truth(cl["xyz"], cl["normals"], 7)
        gcam = np.ascontiguousarray(cam[:, sel])
        ctx.upload_cloud(gt, gn, gcam, vp)
        check(ctx, op, gt, gn, hands)
        # ... then with normals estimated on the device (Cloud::calculateNormals, 1 cm: the smoothed normals of a larger radius
        # leave few full grasps; on some variants none, so this leg asks for label 0 and half flags only)
        ctx.upload_cloud(gt, np.zeros_like(gt), gcam, vp)
        en = ctx.estimate_normals(0.01)
        assert np.array_equal(en, oracle_mod.estimate_normals(gt, gcam, vp, 0.01))
        labels, out = check(ctx, op, gt, en, hands, mixed=False)
        assert (labels == 0).any() and out["half_antipodal"].any()
    finally:
        ctx.close()


# ---- list-capacity tiers ---------------------------------------------------------------------------------------------
def _tier_hands(oracle_mod):
    """1000 hands (125 samples x 8 orientations) of the 30k cloud."""
    cl = synth.make_cloud(1234, 30000)
    si = synth.sample_indices(cl, 125, seed=31)
    return cl, oracle_mod.search(oracle_mod.default_params(15), cl["xyz"], cl["normals"], si).reshape(-1)


def _dense(cl, copies, jitter=0.0003, seed=5):
    """The cloud with `copies` jittered duplicates of every point: hand neighbourhoods (0.11 m) of 6.7 k points on average
    and 12.5 k at most for one copy, 13.5 k / 25 k for three."""
    rng = np.random.RandomState(seed)
    xs = [cl["xyz"]] + [(cl["xyz"] + rng.uniform(-jitter, jitter, cl["xyz"].shape)).astype(np.float32) for _ in range(copies)]
    return np.concatenate(xs), np.concatenate([cl["normals"]] * (copies + 1))


@pytest.mark.parametrize("copies", [1, 3])
def test_list_capacity_tiers(oracle_mod, copies):
    cl, hands = _tier_hands(oracle_mod)
    op = oracle_mod.default_params(15)
    xyz, nrm = _dense(cl, copies)
    ctx = api.Context(api.default_params(15))
    try:
        ctx.upload_cloud(xyz, nrm)
        check(ctx, op, xyz, nrm, hands)
        cap = ctx.fallbacks()["neighbourhood_list_capacity"]
        if copies == 1:
            assert cap == 16384  # the in-place bitonic sort
        else:
            assert cap > 16384 and cap % 4096 == 0  # the global-memory lists
    finally:
        ctx.close()


def test_dense_sparse_dense_on_one_context(oracle_mod):
    cl, hands = _tier_hands(oracle_mod)
    op = oracle_mod.default_params(15)
    xyz, nrm = _dense(cl, 3)
    ctx = api.Context(api.default_params(15))
    try:
        caps = []
        for x, n in ((xyz, nrm), (cl["xyz"], cl["normals"]), (xyz, nrm)):
            ctx.upload_cloud(x, n)
            check(ctx, op, x, n, hands)
            caps.append(ctx.fallbacks()["neighbourhood_list_capacity"])
        assert caps[0] > 16384 and caps[1] == 8192 and caps[2] == caps[0], caps
    finally:
        ctx.close()


# ---- edges -----------------------------------------------------------------------------------------------------------
def _cloud30k_hands(oracle_mod, cl, S=400):
    return oracle_mod.search(oracle_mod.default_params(15), cl["xyz"], cl["normals"], synth.sample_indices(cl, S)).reshape(-1)


def test_edges_of_the_label_path(oracle_mod, cloud30k):
    cl = cloud30k
    op = oracle_mod.default_params(15)
    nfp = op.num_finger_placements
    hands = _cloud30k_hands(oracle_mod, cl)
    v = np.flatnonzero(hands["valid"].astype(bool) & hands["full_antipodal"].astype(bool))
    e = hands.copy()
    # flags set on the way in: the kernel must clear them where the label path stops early
    e["half_antipodal"] = 1
    e["full_antipodal"] = 1
    far, neg, beyond, way_beyond = v[0], v[1], v[2], v[3]
    e["sample"][far] += 5.0  # no ground-truth point within the radius: N = 0
    e["finger_placement_index"][neg] = -1
    e["finger_placement_index"][beyond] = nfp
    e["finger_placement_index"][way_beyond] = 1000
    ctx = api.Context(api.default_params(15))
    try:
        ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
        labels, out = check(ctx, op, cl["xyz"], cl["normals"], e)
        for i in (far, neg, beyond, way_beyond):
            assert labels[i] == 0 and out["half_antipodal"][i] == 0 and out["full_antipodal"][i] == 0
        # n = 1: one hand of label 1, then one of label 0
        l1, o1 = check(ctx, op, cl["xyz"], cl["normals"], hands[v[4]:v[4] + 1], mixed=False)
        l0, o0 = check(ctx, op, cl["xyz"], cl["normals"], e[far:far + 1], mixed=False)
        assert l1.tolist() == [1] and l0.tolist() == [0]
        # n beyond every earlier sample capacity of the context (400 samples -> 450): the buffers are reserved again
        big = np.tile(hands, 9000 // len(hands) + 1)[:9000]
        check(ctx, op, cl["xyz"], cl["normals"], big)
    finally:
        ctx.close()


def test_cameras_do_not_change_labels(oracle_mod, cloud30k):
    cl = cloud30k
    op = oracle_mod.default_params(15)
    hands = _cloud30k_hands(oracle_mod, cl)
    gt, gn, _ = rcs.ground_truth(cl["xyz"], cl["normals"], 3)
    cam, vp = rcs._cams(3, len(gt))
    ctx = api.Context(api.default_params(15))
    try:
        ctx.upload_cloud(gt, gn)
        l1, o1 = check(ctx, op, gt, gn, hands)
        ctx.upload_cloud(gt, gn, cam, vp)
        l3, o3 = check(ctx, op, gt, gn, hands)
        assert np.array_equal(l1, l3) and o1.tobytes() == o3.tobytes()
    finally:
        ctx.close()


def test_noisy_non_unit_normals(oracle_mod, cloud30k):
    cl = cloud30k
    op = oracle_mod.default_params(15)
    hands = _cloud30k_hands(oracle_mod, cl)
    rng = np.random.RandomState(4)
    nrm = (cl["normals"] * rng.uniform(0.6, 1.5, (len(cl["normals"]), 1)) + rng.normal(0, 0.15, cl["normals"].shape)).astype(np.float32)
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() > 0.3
    ctx = api.Context(api.default_params(15))
    try:
        ctx.upload_cloud(cl["xyz"], nrm)
        check(ctx, op, cl["xyz"], nrm, hands)
    finally:
        ctx.close()


def test_detect_after_reevaluate(oracle_mod, cloud30k, lenet15_real):
    """The re-evaluation reuses the search buffers: the next detect on the context must still equal the oracle."""
    cl = cloud30k
    op = oracle_mod.default_params(15)
    si = synth.sample_indices(cl, 64)
    ctx = api.Context(api.default_params(15))
    try:
        ctx.set_lenet_weights(lenet15_real)
        ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
        hands, _ = ctx.detect(si)
        gt, gn, _ = rcs.ground_truth(cl["xyz"], cl["normals"], 5)
        ctx.upload_cloud(gt, gn)
        check(ctx, op, gt, gn, hands.reshape(-1))
        ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
        hands, n_cand = ctx.detect(si)
        ohands, on_cand, _ = oracle_mod.detect(op, cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"], si, lenet15_real)
        assert n_cand == on_cand and n_cand > 0
        a, b = hands.copy(), ohands.copy()
        assert np.abs(a["score"] - b["score"]).max() <= 1e-4
        a["score"] = 0
        b["score"] = 0
        assert a.tobytes() == b.tobytes()
    finally:
        ctx.close()


# ---- independent form ------------------------------------------------------------------------------------------------
def test_device_matches_independent_restatement(oracle_mod):
    """About 200 hands against tests/pyref_hands.reevaluate, which shares no code with the oracle: a misreading of the
    reference that the oracle and the kernel share shows up here."""
    gp, cl, si, _, _ = _variant_inputs("six_placements_wide_fingers", api.default_params)
    op = _variant_inputs("six_placements_wide_fingers", oracle_mod.default_params)[0]
    hands = oracle_mod.search(op, cl["xyz"], cl["normals"], si).reshape(-1)
    pick = np.concatenate([np.flatnonzero(hands["valid"].astype(bool))[:160], np.flatnonzero(~hands["valid"].astype(bool))[:40]])
    recs = hands[np.sort(pick)]
    gt, _, sel = rcs.ground_truth(cl["xyz"], cl["normals"], 7)
    ctx = api.Context(gp)
    try:
        for xyz, nrm in ((cl["xyz"], cl["normals"]), (gt, cl["normals"][sel])):
            ctx.upload_cloud(xyz, nrm)
            labels, out = check(ctx, op, xyz, nrm, recs)
            pl, ph, pf = pyref_hands.reevaluate(op, xyz, nrm, recs)
            assert np.array_equal(labels, pl)
            assert np.array_equal(out["half_antipodal"].astype(bool), ph) and np.array_equal(out["full_antipodal"].astype(bool), pf)
    finally:
        ctx.close()
