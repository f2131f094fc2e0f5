"""Every composed entry of the library — detect_select, detect_samples, images_given / score_given, detect_batch (with and
without gpd_hip_reserve), detect_batch_multi, detect_sharded, detect_sis, label_view — on every variant of tests/ref_cases.py:
1 / 3 / 12 / 15 channels, 4 to 24 slots per sample, the hand and image geometries up to the general shadow kernel, 1 to 12
cameras, off-lattice clouds.  The expectations are composed from the oracle alone (tests/entry_cases.py; tests/test_entry_cases.py
proves them non-empty).  In LENET_F32_CHAIN mode every record array compares byte for byte, score bits included; detect_select
runs once more in LENET_SPLIT mode, within BASELINE.json's 1e-4 of the oracle."""
import numpy as np
import pytest

import entry_cases as ec
import label_view_cases as lvc
import ref_cases as rcs
from gpd_amd import api

pytestmark = pytest.mark.gpu

SPLIT_TOL = 1e-4  # BASELINE.json: scores of the default mode against the oracle, trained-magnitude weights
ROUTES = {"wide_image_volume": (1, 1), "huge_image_volume": (2, 2)}  # (window_class, set_mode) the image volume selects


def _same(got, want, what, score_tol=None):
    """`what` = (variant, entry, detail).  Byte for byte; with score_tol the scores within it and every other byte equal."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = rcs.records_equal(got, want)
    assert not bad, (what, bad)
    a, b = got, want
    if score_tol is not None:
        if got.size:
            err = float(np.abs(got["score"].astype(np.float64) - want["score"]).max())
            assert err <= score_tol, (what, "score", err)
        a, b = got.copy(), want.copy()
        a["score"] = 0
        b["score"] = 0
    assert a.tobytes() == b.tobytes(), (what, [f for f in got.dtype.names if a[f].tobytes() != b[f].tobytes()])


def _context(p, w, mode=api.LENET_F32_CHAIN):
    ctx = api.Context(p)
    ctx.set_lenet_weights(w)
    ctx.set_lenet_mode(mode)
    return ctx


def _upload(ctx, cl):
    ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])


def _check_batch(name, entry, got, want, k):
    assert len(got) == len(want) == 3, (name, entry, len(got))
    for j, (g, w) in enumerate(zip(got, want)):
        what = (name, entry, "job %d, num_selected %d" % (j, k))
        assert (g[1], g[2]) == (w["n_sets"], w["n_cand"]), (what, g[1:3], (w["n_sets"], w["n_cand"]))
        _same(g[0], ec.selected(w, k), what)
    assert got[2][2] == 0 and len(got[2][0]) == 0, (name, entry, "the job without samples")


def _copies(res):
    return [(h.copy(), ns, nc) for h, ns, nc, _ in res]


@pytest.mark.parametrize("name", sorted(rcs.VARIANTS))
def test_every_entry_on_the_variant(oracle_mod, name):
    om = oracle_mod
    p, cl, si, w = ec.inputs(name, api.default_params)
    slots, ncam = ec.slots(p), cl["cam_source"].shape[0]
    clouds, samples = ec.batch_jobs(name, api.default_params)
    ctx = _context(p, w)
    other = None
    try:
        assert ctx.n_slots == slots
        gt, gn = ec.ground_truth(name)
        ctx.upload_ground_truth(gt, gn)  # for step 6: it must outlive every call in between
        _upload(ctx, cl)

        # ---- 1. detect, detect_select, detect_samples -------------------------------------------------------------------
        d = ec.detect(om, name)
        hands, nc = ctx.detect(si)
        assert nc == d["n_cand"], (name, "detect", nc, d["n_cand"])
        _same(hands, d["hands"], (name, "detect", ""))
        first, ns, nc = ctx.detect_select(si, 0)
        first = first.copy()
        assert (ns, nc) == (d["n_sets"], d["n_cand"]), (name, "detect_select", ns, nc)
        _same(first, ec.selected(d, 0), (name, "detect_select", "num_selected 0"))
        top, ns, nc = ctx.detect_select(si, ec.SELECT_K)
        assert (ns, nc) == (d["n_sets"], d["n_cand"]), (name, "detect_select", ns, nc)
        _same(top, ec.selected(d, ec.SELECT_K), (name, "detect_select", "num_selected %d" % ec.SELECT_K))
        ctx.set_lenet_mode(api.LENET_SPLIT)
        split, _, nc = ctx.detect_select(si, 0)
        ctx.set_lenet_mode(api.LENET_F32_CHAIN)
        assert nc == d["n_cand"]
        _same(split, ec.selected(d, 0), (name, "detect_select", "LENET_SPLIT"), score_tol=SPLIT_TOL)
        ds = ec.detect_samples(om, name)
        hands, nc = ctx.detect_samples(ec.sample_points(name))
        assert nc == ds["n_cand"], (name, "detect_samples", nc, ds["n_cand"])
        _same(hands, ds["hands"], (name, "detect_samples", ""))

        # ---- 2. images_given / score_given ------------------------------------------------------------------------------
        sets = ec.given_sets(om, name)
        for which in ("a", "b"):
            assert api.given_check(p, sets[which]) is None, (name, "given_check", which)
            for base in ec.LCG_BASES:
                what = (name, "images_given", "hand sets (%s), lcg_base %d" % (which, base))
                want = ec.given(om, name, which, base)
                img, cand, draws = ctx.images_given(sets[which], lcg_base=base)
                assert np.array_equal(cand, want["cand"]), what
                assert draws == want["draws"], (what, draws, want["draws"])
                assert img.shape == want["images"].shape, (what, img.shape)
                diff = np.flatnonzero((img != want["images"]).reshape(len(cand), -1).any(axis=1))
                assert img.tobytes() == want["images"].tobytes(), (what, len(diff), diff[:10], cand[diff[:10]] // slots)
                what = (name, "score_given") + what[2:]
                out, scores, cand, draws = ctx.score_given(sets[which], lcg_base=base)
                assert np.array_equal(cand, want["cand"]) and draws == want["draws"], (what, draws, want["draws"])
                assert scores.tobytes() == want["scores"].tobytes(), (what, float(np.abs(scores - want["scores"]).max()) if len(cand) else 0.0)
                scored = sets[which].copy()
                scored.reshape(-1)["score"][want["cand"]] = want["scores"]
                _same(out, scored, what)
        if name in ROUTES:  # the composed entry reached the shadow kernels of the volume's window class with its own plan
            _, info = ctx.image_routes()
            assert info["candidates"] == len(cand), (name, "score_given", info)
            assert (info["window_class"], info["set_mode"]) == ROUTES[name], (name, "score_given", info)

        # ---- 3. detect_batch: three jobs, then after gpd_hip_reserve on a fresh context --------------------------------
        b = ec.batch(om, name)
        assert b[1]["n_cand"] > 0 and b[2]["n_cand"] == 0
        single = {}
        for k in (0, ec.SELECT_K):
            got = ctx.detect_batch(clouds, samples, k)
            _check_batch(name, "detect_batch", got, b, k)
            single[k] = _copies(got)
            rev = ctx.detect_batch(clouds[::-1], samples[::-1], k)[::-1]
            for j, (g, r) in enumerate(zip(single[k], rev)):
                assert g[1:] == r[1:3] and g[0].tobytes() == r[0].tobytes(), (name, "detect_batch", "reversed order, job %d, num_selected %d" % (j, k),
                                                                             rcs.records_equal(g[0], r[0]) if len(g[0]) == len(r[0]) else "length")
        other = _context(p, w)
        other.reserve(max_points=max(len(c["xyz"]) for c in clouds), max_cams=ncam, max_samples=rcs.NUM_SAMPLES)
        got = other.detect_batch(clouds, samples, 0)
        allocs = [a for _, a in other.last_batch_timeline]
        assert allocs == [0, 0, 0], (name, "reserve + detect_batch", "buffer growths per job", allocs, slots, ncam)
        _check_batch(name, "reserve + detect_batch", got, b, 0)

        # ---- 4. detect_batch_multi, detect_sharded over two contexts on the one device ------------------------------------
        for k in (0, ec.SELECT_K):
            got = ctx.detect_batch_multi([other], clouds, samples, k)
            assert len(got) == 3
            for j, (g, r) in enumerate(zip(got, single[k])):
                what = (name, "detect_batch_multi", "job %d, num_selected %d" % (j, k))
                assert (g[1], g[2]) == r[1:], (what, g[1:3], r[1:])
                _same(g[0], r[0], what)
        got, info = ctx.detect_sharded([other], cl, si, [5])
        assert sum(i[0] for i in info) == d["n_sets"] and sum(i[1] for i in info) == d["n_cand"], (name, "detect_sharded", info)
        assert info[0][2] == 0 and info[1][2] == info[0][3], (name, "detect_sharded", "lcg_base of shard 1 != lcg_draws of shard 0", info)
        assert (info[0][3], info[1][3]) == ec.shard_draws(om, name, 5), (name, "detect_sharded", info, ec.shard_draws(om, name, 5))
        _same(got, first, (name, "detect_sharded", "split [5]"))

        # ---- 5. detect_sis (the batch entries replaced the uploaded cloud) ------------------------------------------------
        _upload(ctx, cl)
        pred = ec.sis_predict(om, name)
        got = ctx.detect_sis(si, num_iterations=ec.SIS["rounds"], num_samples=ec.SIS["per"], sampling_method=ec.SIS["method"],
                             seed=ec.SIS["seed"], min_score=ec.SIS["min_score"])
        assert got["rounds_run"] == ec.SIS["rounds"], (name, "detect_sis", got["rounds_run"])
        assert got["samples"].tobytes() == pred["samples"].tobytes(), (name, "detect_sis", "samples of the rounds")
        assert got["round_counts"][1:, 2:].tolist() == pred["consumed"].tolist(), (name, "detect_sis", got["round_counts"].tolist())
        rep = ec.sis_replay(om, name, got["samples"])
        assert got["round_counts"][:, 0].tolist() == rep["live"] and got["round_counts"][:, 1].tolist() == rep["candidates"], \
            (name, "detect_sis", got["round_counts"].tolist(), rep["live"], rep["candidates"])
        assert got["centres"].tobytes() == rep["centres"].tobytes(), (name, "detect_sis", "centres")
        _same(got["hands"], rep["hands"], (name, "detect_sis", "records"))
        _same(got["hands"], pred["hands"], (name, "detect_sis", "records against the prediction"))

        # ---- 6. label_view ------------------------------------------------------------------------------------------------
        view = ctx.label_view(ec.view_rounds(name), ec.MIN_POSITIVES, ec.MAX_GRASPS_PER_VIEW, want_all_labels=True)
        lvc.assert_view(view, ec.view(om, name), (name, "label_view"))

        # ---- 7. no entry left state behind that changes another ----------------------------------------------------------
        again, ns, nc = ctx.detect_select(si, 0)
        assert (ns, nc) == (d["n_sets"], d["n_cand"]), (name, "detect_select after every entry", ns, nc)
        _same(again, first, (name, "detect_select after every entry", ""))
    finally:
        ctx.close()
        if other is not None:
            other.close()
