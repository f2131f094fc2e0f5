"""The walk of tests/test_gpu_entries_by_variant.py with gpd_hip_set_shadow_jitter ON, over the nine variants of
entry_cases.JITTER_VARIANTS: every composed entry — detect, detect_select, detect_samples, images_given / score_given at both
stream positions, detect_batch (with and without gpd_hip_reserve), detect_batch_multi, detect_sharded, detect_sis, label_view —
against expectations composed from the oracle alone with ITS statement of the policy on (oracle/gpd_oracle.cpp,
gpd_oracle_set_shadow_jitter; tests/test_oracle_shadow_jitter.py checks that statement, tests/test_entry_cases.py that the
expectations differ from those of the setting off).  Both contexts get the setting before any other call, the second one
before gpd_hip_reserve.

The variants take every window-class transition the setting causes (image::window_class of gpd_amd/csrc/image_model.h, two
more voxels on each side; the literals below are worked out from that formula by hand): the stock geometry leaves the default
windows for the wide ones, other_image_volume stays with one voxel to spare, deep_hand stays wide with more reach,
wide_image_volume leaves the wide windows for the general kernel with a set region SMALLER than the wide one's, and
huge_image_volume's region grows.  At the end the setting is switched off on the same context and detect_select must return
the jitter-free records: on wide_image_volume that is the general kernel -> wide windows return over buffers sized for both.
default_c12 has no shadow channel: the walk runs with the setting on against the expectations of the setting off."""
import numpy as np
import pytest

import entry_cases as ec
import label_view_cases as lvc
import ref_cases as rcs
from gpd_amd import api
from test_gpu_entries_by_variant import SPLIT_TOL, _check_batch, _context, _copies, _same, _upload

pytestmark = pytest.mark.gpu

SEED = ec.JITTER_SEED
# variant -> ((window_class, set_sr) with the setting off, (window_class, set_sr) with it on)
STOCK = ((0, 43), (1, 64))
WINDOWS = {
    "default_c15": STOCK,
    "default_c12": STOCK,  # the model of the geometry; the device keeps class 0, there is no shadow to window
    "three_axes": STOCK,
    "twelve_cameras": STOCK,
    "offlattice_two_cameras": STOCK,
    "other_image_volume": ((0, 43), (0, 43)),  # need_win = 45 of 46
    "deep_hand": ((1, 64), (1, 64)),           # reach 44 -> 46
    "wide_image_volume": ((1, 64), (2, 55)),   # the general kernel, a set region of 110 voxels under the wide region's 128
    "huge_image_volume": ((2, 60), (2, 62)),
}


def test_the_table_names_the_nine_variants():
    assert sorted(WINDOWS) == sorted(ec.JITTER_VARIANTS) and len(WINDOWS) == 9


@pytest.mark.parametrize("name", ec.JITTER_VARIANTS)
def test_every_entry_on_the_variant_with_the_shadow_jitter_on(oracle_mod, name):
    om = oracle_mod
    p, cl, si, w = ec.inputs(name, api.default_params)
    slots, ncam = ec.slots(p), cl["cam_source"].shape[0]
    has_shadow = p.image_num_channels == 15
    clouds, samples = ec.batch_jobs(name, api.default_params)
    # the host model of both settings is the table's
    for setting in (0, 1):
        m = api.image_model(p, setting)
        assert (m["window_class"], m["set_sr"]) == WINDOWS[name][setting], (name, "image_model", setting, m["window_class"], m["set_sr"])
    want_class = WINDOWS[name][1][0] if has_shadow else 0
    off = ec.detect(om, name)
    ctx = _context(p, w)
    other = None
    # without a shadow channel the expectations are those of the setting off (seed None: the oracle stays off)
    with ec.jitter(om, SEED if has_shadow else None):
        try:
            ctx.set_shadow_jitter(True, SEED)
            assert ctx.n_slots == slots
            gt, gn = ec.ground_truth(name)
            ctx.upload_ground_truth(gt, gn)  # for step 6: it must outlive every call in between
            _upload(ctx, cl)

            # ---- 1. detect, detect_select, detect_samples ---------------------------------------------------------------
            d = ec.detect(om, name)
            assert (d is off) == (not has_shadow)
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

            # ---- 2. images_given / score_given at both stream positions --------------------------------------------------
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
            # the composed entry ran the shadow kernels of the window class the setting selects
            _, info = ctx.image_routes()
            print("%s: window_class on the device with the setting on %d (table %d), set_mode %d, status %d"
                  % (name, info["window_class"], want_class, info["set_mode"], info["status"]))
            assert info["candidates"] == len(cand) and info["status"] == 0, (name, "score_given", info)
            assert info["window_class"] == want_class, (name, "score_given", info)
            if has_shadow:
                assert info["window_class"] == api.image_model(p, 1)["window_class"] == info["set_mode"], (name, "score_given", info)

            # ---- 3. detect_batch: three jobs, then after gpd_hip_reserve on a fresh context with the setting on ------------
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
            other.set_shadow_jitter(True, SEED)  # before reserve: gpd_hip_reserve sizes for the setting in force
            other.reserve(max_points=max(len(c["xyz"]) for c in clouds), max_cams=ncam, max_samples=rcs.NUM_SAMPLES)
            got = other.detect_batch(clouds, samples, 0)
            allocs = [a for _, a in other.last_batch_timeline]
            assert allocs == [0, 0, 0], (name, "reserve + detect_batch", "buffer growths per job", allocs, slots, ncam)
            _check_batch(name, "reserve + detect_batch", got, b, 0)

            # ---- 4. detect_batch_multi, detect_sharded over two contexts on the one device --------------------------------
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

            # ---- 5. detect_sis (the batch entries replaced the uploaded cloud) --------------------------------------------
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

            # ---- 6. label_view --------------------------------------------------------------------------------------------
            view = ctx.label_view(ec.view_rounds(name), ec.MIN_POSITIVES, ec.MAX_GRASPS_PER_VIEW, want_all_labels=True)
            lvc.assert_view(view, ec.view(om, name), (name, "label_view"))

            # ---- 7. no entry left state behind that changes another -------------------------------------------------------
            again, ns, nc = ctx.detect_select(si, 0)
            assert (ns, nc) == (d["n_sets"], d["n_cand"]), (name, "detect_select after every entry", ns, nc)
            _same(again, first, (name, "detect_select after every entry", ""))
            assert ctx.image_routes()[1]["window_class"] == want_class

            # ---- 8. off again on the same context: the records of a context that never had it on ---------------------------
            ctx.set_shadow_jitter(False)
            back, ns, nc = ctx.detect_select(si, 0)
            assert (ns, nc) == (off["n_sets"], off["n_cand"]), (name, "detect_select after the setting went off", ns, nc)
            _same(back, ec.selected(off, 0), (name, "detect_select after the setting went off", ""))
            _, info = ctx.image_routes()
            print("%s: window_class on the device with the setting off again %d (table %d)" % (name, info["window_class"], WINDOWS[name][0][0]))
            assert info["status"] == 0 and info["window_class"] == WINDOWS[name][0][0] == api.image_model(p, 0)["window_class"], (name, info)
            if has_shadow:
                assert back["score"].tobytes() != first["score"].tobytes(), (name, "the setting decided no score")
        finally:
            ctx.close()
            if other is not None:
                other.close()
