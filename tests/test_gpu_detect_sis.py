"""gpd_hip_detect_sis (SequentialImportanceSampling::detectGrasps with the rounds kept on the device) against the oracle's own
entries and the Python restatement of the draws (tests/sis_cases.py, tests/pyref_sis.py), against the host-only model entries,
and against the same samples fed through the existing public calls one at a time."""
import ctypes as C

import numpy as np
import pytest

import pyref_sis
import ref_cases as rcs
import sis_cases as sc
from gpd_amd import api

pytestmark = pytest.mark.gpu

DRAW_THREADS, CENTRE_TILE = 512, 512  # kSisDrawThreads, kSisCentreTile (gpd_amd/csrc/gpd_internal.h)
FIELDS = ("sample", "frame", "position", "top", "bottom", "center", "grasp_width", "finger_placement_index", "set_index", "slot", "valid",
          "half_antipodal", "full_antipodal")


def _context(weights, channels=15, cams=2, **over):
    cl, cam, vp, init = sc.scene(cams)
    ctx = api.Context(rcs.set_params(api.default_params(channels), **over))
    ctx.set_lenet_weights(weights)
    ctx.upload_cloud(cl["xyz"], cl["normals"], cam, vp)
    return ctx, cl, cam, vp, init


def _run(ctx, init, method=0, **kw):
    a = dict(num_iterations=sc.ROUNDS, num_samples=sc.PER, prob_rand_samples=sc.PROB_RAND, sigma=sc.SIGMA, sampling_method=method,
             min_score=sc.MIN_SCORE, seed=sc.SEED[method])
    a.update(kw)
    return ctx.detect_sis(init, **a)


def _records_equal(got, want, what, scores_tol=None):
    assert len(got) == len(want), (what, len(got), len(want))
    bad = [f for f in FIELDS if not np.array_equal(got[f], want[f])]
    assert not bad, (what, bad)
    if scores_tol is None:
        assert got["score"].tobytes() == want["score"].tobytes(), what
        assert got.tobytes() == want.tobytes(), what
    elif len(got):
        err = float(np.abs(got["score"].astype(np.float64) - want["score"]).max())
        print("%s: %d records, largest score difference %.3g" % (what, len(got), err))
        assert err <= scores_tol, (what, err)


def _assert_draws_equal_model(got, cl, init, method, seed, workspace=sc.WS_ALL, prob=sc.PROB_RAND, sigma=sc.SIGMA, uniform_list="init"):
    """samples_out of every round == api.sis_select on the returned centres cut to that round's length + api.sis_proposals."""
    per = got["samples"].shape[1]
    nr = pyref_sis.num_rand_samples(prob, per)
    ng = per - nr
    before = sc.centres_before(got["round_counts"])
    lst = init if uniform_list == "init" else uniform_list
    for r in range(got["rounds_run"]):
        used_g, used_u = int(got["round_counts"][1 + r, 2]), int(got["round_counts"][1 + r, 3])
        want = api.sis_select(got["centres"][: before[r]], api.sis_proposals(seed, r, 0, 0, used_g, sigma), api.sis_proposals(seed, r, 1, 0, used_u),
                              lst, cl["xyz"], workspace, method, ng, nr)
        assert want["shortfall"] == 0 and want["consumed"].tolist() == [used_g, used_u], (r, want["consumed"], used_g, used_u)
        assert got["samples"][r].tobytes() == want["samples"].tobytes(), "round %d" % r
        if used_g > 0:  # one proposal less does not fill the list: the count is the one the sequential loop stops at
            short = api.sis_select(got["centres"][: before[r]], api.sis_proposals(seed, r, 0, 0, used_g - 1, sigma),
                                   api.sis_proposals(seed, r, 1, 0, used_u), lst, cl["xyz"], workspace, method, ng, nr)
            assert short["shortfall"] == 1


# ---- 1. replay through the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_inliers", [0, 1])
@pytest.mark.parametrize("method", [0, 1])
def test_replay_through_the_oracle(oracle_mod, lenet15_real, method, min_inliers):
    ctx, cl, cam, vp, init = _context(lenet15_real)
    try:
        got = _run(ctx, init, method, min_inliers=min_inliers)
        ctx.set_lenet_mode(api.LENET_F32_CHAIN)
        chain = _run(ctx, init, method, min_inliers=min_inliers)
    finally:
        ctx.close()
    assert got["rounds_run"] == sc.ROUNDS and got["samples"].shape == (sc.ROUNDS, sc.PER, 3)
    p = oracle_mod.default_params(15)
    want = sc.replay(oracle_mod, p, cl, cam, vp, init, got["samples"], lenet15_real, sc.MIN_SCORE, min_inliers)
    # what keeps the comparison from passing vacuously
    assert all(n >= 1 for n in want["live"]), want["live"]
    assert len(want["hands"]) > 5
    if method == 1:
        assert (got["round_counts"][1:, 2] > sc.PER - pyref_sis.num_rand_samples(sc.PROB_RAND, sc.PER)).any(), got["round_counts"].tolist()
    assert got["round_counts"][:, 0].tolist() == want["live"] and got["round_counts"][:, 1].tolist() == want["candidates"]
    assert got["num_sets"] == sum(want["live"]) and got["num_candidates"] == sum(want["candidates"])
    assert got["centres"].tobytes() == want["centres"].tobytes()
    _records_equal(chain["hands"], want["hands"], "f32 chain, method %d, min_inliers %d" % (method, min_inliers))
    _records_equal(got["hands"], want["hands"], "split mode, method %d, min_inliers %d" % (method, min_inliers), scores_tol=1e-4)
    assert chain["samples"].tobytes() == got["samples"].tobytes()
    # the whole call predicted without the library: the draws of pyref_sis on the oracle's centres
    pred = sc.predict(oracle_mod, p, cl, cam, vp, init, lenet15_real, sc.SEED[method], method, min_inliers=min_inliers)
    assert got["samples"].tobytes() == pred["samples"].tobytes()
    assert got["round_counts"][1:, 2:].tolist() == pred["consumed"].tolist()
    # per round only small words cross PCIe; the records leave once
    small = 64 * (2 * (1 + sc.ROUNDS) + 4)
    assert 0 < got["d2h_bytes"] <= len(got["hands"]) * 176 + got["samples"].nbytes + got["centres"].nbytes + small + 4096, got["d2h_bytes"]
    print("detect_sis: %d sets, %d candidates, %d hands, %d bytes to the host, stage ms %s"
          % (got["num_sets"], got["num_candidates"], got["num_hands"], got["d2h_bytes"], ["%.3f" % m for m in got["stage_ms"]]))


# ---- 2. the draws equal the model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1])
def test_draws_equal_the_model(lenet15_real, method):
    ctx, cl, cam, vp, init = _context(lenet15_real)
    try:
        got = _run(ctx, init, method)
    finally:
        ctx.close()
    assert got["rounds_run"] == sc.ROUNDS
    _assert_draws_equal_model(got, cl, init, method, sc.SEED[method])


# ---- 3. equal to the composed route ----------------------------------------------------------------------------------------
def _composed(ctx, om, init, rounds, min_score):
    """The same samples through the public calls, as the host loop and pruneGraspCandidates compose them."""
    p = om.default_params(ctx.params.image_num_channels)
    sets = [sc.live_sets(om, p, ctx.search(init))]
    for r in rounds:
        sets.append(sc.live_sets(om, p, ctx.search_samples(r)))
    allh = np.concatenate([s for s in sets if len(s)])
    fresh = ctx.search_samples(allh[:, 0]["sample"])  # the collected list no longer matches the device's search state
    assert len(fresh) == len(allh)
    fresh["valid"] = allh["valid"]
    fresh["set_index"] = np.arange(len(fresh), dtype=np.int32)[:, None]
    _, cand = ctx.images(fresh, download=False)
    scores = ctx.score(None, n=len(cand))
    recs = fresh.reshape(-1)[cand].copy()
    recs["score"] = scores
    return recs[scores > np.float64(min_score)]


@pytest.mark.parametrize("method", [0, 1])
def test_equal_to_the_composed_route(oracle_mod, lenet15_real, method):
    ctx, cl, cam, vp, init = _context(lenet15_real)
    try:
        got = _run(ctx, init, method)
        want = _composed(ctx, oracle_mod, init, got["samples"], sc.MIN_SCORE)
    finally:
        ctx.close()
    assert len(want) > 5
    _records_equal(got["hands"], want, "composed route, method %d" % method)  # record bytes and score bits: the shadow stream ran on


# ---- 4. proposal blocks ---------------------------------------------------------------------------------------------------
def test_proposal_blocks(lenet15_real):
    ctx, cl, cam, vp, init = _context(lenet15_real)
    ws = (-1.0, float(np.median(cl["xyz"][init, 0])), -1.0, 1.0, -1.0, 1.0)  # cuts away about half of the uniform source
    inside = cl["xyz"][init, 0] <= np.float32(ws[1])
    assert 0.3 < inside.mean() < 0.7
    try:
        small = _run(ctx, init, 1, workspace=ws, proposal_block=8)
        default = _run(ctx, init, 1, workspace=ws)
    finally:
        ctx.close()
    nr = pyref_sis.num_rand_samples(sc.PROB_RAND, sc.PER)
    assert small["rounds_run"] == sc.ROUNDS
    assert (small["round_counts"][1:, 3] > nr).any()             # a uniform proposal was rejected
    assert (small["round_counts"][1:, 2:].max(axis=1) > 8).all()  # more than one block per round
    for k in ("hands", "samples", "centres", "round_counts"):
        assert small[k].tobytes() == default[k].tobytes(), k
    _assert_draws_equal_model(small, cl, init, 1, sc.SEED[1], workspace=ws)
    assert np.all(small["samples"][:, sc.PER - nr:, 0] <= ws[1])


# ---- 5. tile and workgroup edges of sis_draw_kernel -------------------------------------------------------------------------
def test_draw_kernel_tile_and_workgroup_edges(lenet15_real):
    """Rounds of DRAW_THREADS + 1 Gaussian samples from blocks of DRAW_THREADS + 1 proposals: every block is one full step of the
    workgroup and a step of one lane, and under method 1 the rejections make every round take several blocks.  The centre list
    crosses CENTRE_TILE between the first and the second round."""
    ctx, cl, cam, vp, _ = _context(lenet15_real)
    init = np.flatnonzero(cl["is_object"])[::5][:560].astype(np.int32)
    try:
        got = _run(ctx, init, 1, num_iterations=2, num_samples=DRAW_THREADS + 1, prob_rand_samples=0.0, proposal_block=DRAW_THREADS + 1, seed=3)
    finally:
        ctx.close()
    before = sc.centres_before(got["round_counts"])
    print("centres before the rounds:", before, "proposals consumed:", got["round_counts"][1:, 2].tolist())
    assert got["rounds_run"] == 2 and 0 < before[0] <= CENTRE_TILE < before[1] and before[1] % CENTRE_TILE != 0
    assert (got["round_counts"][1:, 2] > DRAW_THREADS + 1).all()
    _assert_draws_equal_model(got, cl, init, 1, 3, prob=0.0)


# ---- 6. edges -------------------------------------------------------------------------------------------------------------
def test_no_iterations_equals_detect_select(lenet15_real):
    ctx, cl, cam, vp, init = _context(lenet15_real)
    try:
        min_score = -4.0
        got = _run(ctx, init, 0, num_iterations=0, num_samples=0, min_score=min_score)
        hands, n_sets, n_cand = ctx.detect_select(init, 0)
        hands = hands.copy()
    finally:
        ctx.close()
    assert got["rounds_run"] == 0 and got["num_candidates"] == n_cand and got["samples"].shape[0] == 0
    # detect_select numbers a record's set among ALL hand sets of the search, detect_sis among the live ones
    _, live_index = np.unique(hands["set_index"], return_inverse=True)
    hands["set_index"] = live_index.astype(np.int32)
    want = hands[hands["score"] > np.float64(min_score)]
    assert 5 < len(want) < n_cand
    _records_equal(got["hands"], want, "num_iterations = 0")
    assert got["num_sets"] == live_index.max() + 1 <= n_sets


def test_initial_pass_without_a_live_set(lenet15_real):
    # every hand of the initial pass falls outside workspace_grasps: hand sets, but none that keeps a valid hand
    ctx, cl, cam, vp, init = _context(lenet15_real, workspace_grasps=[5.0, 6.0, 5.0, 6.0, 5.0, 6.0])
    try:
        got = _run(ctx, init, 1)
        assert (got["rounds_run"], got["num_sets"], got["num_candidates"], got["num_hands"]) == (0, 0, 0, 0)
        assert got["round_counts"].tolist() == [[0, 0, 0, 0]] * (1 + sc.ROUNDS)
        none = ctx.detect_sis(np.zeros(0, np.int32), 2, 8)  # no initial samples at all
        assert (none["rounds_run"], none["num_hands"]) == (0, 0)
    finally:
        ctx.close()


def test_three_channels(oracle_mod):
    w = rcs.weights(3, trained_magnitude=True)
    ctx, cl, cam, vp, init = _context(w, channels=3, cams=1)
    try:
        ctx.set_lenet_mode(api.LENET_F32_CHAIN)
        got = _run(ctx, init, 1, num_iterations=2)
    finally:
        ctx.close()
    want = sc.replay(oracle_mod, oracle_mod.default_params(3), cl, cam, vp, init, got["samples"], w, sc.MIN_SCORE, 0)
    assert got["rounds_run"] == 2 and len(want["hands"]) > 5
    _records_equal(got["hands"], want["hands"], "C = 3 (no shadow draws)")


def test_every_sample_uniform(lenet15_real):
    ctx, cl, cam, vp, init = _context(lenet15_real)
    try:
        got = _run(ctx, init, 1, prob_rand_samples=1.0)
    finally:
        ctx.close()
    assert got["rounds_run"] == sc.ROUNDS and (got["round_counts"][1:, 2] == 0).all() and (got["round_counts"][1:, 3] == sc.PER).all()
    _assert_draws_equal_model(got, cl, init, 1, sc.SEED[1], prob=1.0)
    pts = cl["xyz"][init].astype(np.float64)
    assert all((pts == s).all(axis=1).any() for s in got["samples"].reshape(-1, 3))


def _job(init, **over):
    j = api.SisJob()
    hands = np.zeros(4096, api.HAND_DTYPE)
    j.sample_indices, j.num_init_samples = api._ptr(init), len(init)
    j.num_iterations, j.num_samples, j.sampling_method = 1, 8, 0
    j.prob_rand_samples, j.sigma, j.min_score = 0.3, 0.02, -300.0
    j.workspace = (C.c_double * 6)(*sc.WS_ALL)
    j.hands, j.capacity = api._ptr(hands), len(hands)
    for k, v in over.items():
        setattr(j, k, v)
    return j, hands


def test_capacity_and_refusals(lenet15_real):
    ctx, cl, cam, vp, init = _context(lenet15_real)
    f = api.lib().gpd_hip_detect_sis
    try:
        with pytest.raises(api.GpdHipError, match="error -3"):
            _run(ctx, init, 0, capacity=1)
        assert ctx.last_sis_num_hands > 5  # how many there were
        j, keep = _job(init)
        assert f(ctx._h, C.byref(j)) == 0 and j.num_hands > 0 and j.rounds_run == 1
        bad_index = init.copy()
        bad_index[3] = len(cl["xyz"])
        for over in (dict(sample_indices=api._ptr(bad_index)), dict(num_samples=0), dict(prob_rand_samples=-0.1), dict(prob_rand_samples=1.5),
                     dict(sigma=0.0), dict(sigma=-1.0), dict(sampling_method=2), dict(sampling_method=-1), dict(hands=None),
                     dict(num_iterations=-1), dict(capacity=-1)):
            j, keep = _job(init, **over)
            assert f(ctx._h, C.byref(j)) == -1, over
            assert j.num_hands == 0
        assert f(ctx._h, None) == -1
        j, keep = _job(init, hands=None, capacity=0)  # nothing asked for: the count alone
        assert f(ctx._h, C.byref(j)) == -3 and j.num_hands > 0
        # the context is still usable
        j, keep = _job(init)
        assert f(ctx._h, C.byref(j)) == 0
    finally:
        ctx.close()
    no_weights = api.Context(api.default_params(15))
    try:
        no_weights.upload_cloud(cl["xyz"], cl["normals"], cam, vp)
        j, keep = _job(init)
        assert f(no_weights._h, C.byref(j)) == -4
    finally:
        no_weights.close()
    no_cloud = api.Context(api.default_params(15))
    try:
        no_cloud.set_lenet_weights(lenet15_real)
        j, keep = _job(init)
        assert f(no_cloud._h, C.byref(j)) == -4
    finally:
        no_cloud.close()


# ---- 7. run to run and aftermath ------------------------------------------------------------------------------------------
def test_run_to_run_and_aftermath(lenet15_real):
    ctx, cl, cam, vp, init = _context(lenet15_real)
    try:
        before, n_before = ctx.detect(init)
        before = before.copy()
        a = _run(ctx, init, 1, min_inliers=1)
        b = _run(ctx, init, 1, min_inliers=1)
        after, n_after = ctx.detect(init)
    finally:
        ctx.close()
    for k in ("hands", "samples", "centres", "round_counts"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert len(a["hands"]) > 5
    assert n_before == n_after and before.tobytes() == after.tobytes()
