"""The Caffe recipe on the device (gpd_train_recipe): the network without conv ReLUs against float64 autograd, the
first-maximum routing on ties, Caffe's SGD rule with its learning-rate policies and multipliers against the rule written out in
float64, the update counter, resuming from a solver state, eval, the way into scoring through gpd_amd.eigen_export, the tool,
and that a trainer without a recipe is untouched.  References: train_caffe_ref.py; the yardstick and its bound are
train_ref.py's (truth float64, e32 = the larger error of two torch float32 runs, allowance FACTOR * e32 with check_gradients'
floors).  Measured figures: DESIGN §11, "The Caffe recipe".
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import train_caffe_ref as cr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Rig:
    """A context and a trainer on it, closed in order.  recipe: None (no recipe), a gpd_train_recipe, or "caffe"."""

    def __init__(self, C, recipe="caffe", **kw):
        from gpd_amd import api
        if isinstance(recipe, str):
            recipe = api.train_default_recipe(1)
            kw.setdefault("lr", api.CAFFE_BASE_LR)
        self.ctx = api.Context(api.default_params(C))
        try:
            self.trainer = api.Trainer(self.ctx, recipe=recipe, **kw)
        except Exception:
            self.ctx.close()
            raise

    def __enter__(self):
        return self.trainer

    def __exit__(self, *exc):
        self.trainer.close()
        self.ctx.close()


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


def _batch(B, n=70):
    """The last B images of the resident set in an order that is not the stored one"""
    idx = (n - 1 - np.arange(B)).astype(np.int32)
    idx[: B // 2] = idx[: B // 2][::-1]
    return idx


# ---- 1. gradients and loss -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,B,max_batch", [(1, 1, 64), (3, 5, 64), (15, 70, 70)])
def test_gradients_against_float64_autograd(C, B, max_batch):
    img, lab, st = cr.images(C), cr.labels(), cr.xavier_state(C)
    idx = _batch(B)
    g64, l64, e32, el32 = cr.yardstick(st, img[idx], lab[idx])
    with _Rig(C, max_batch=max_batch) as t:
        t.set_state(st)
        t.set_data(img, lab)
        got, loss = t.gradients(idx)
        again, loss2 = t.gradients(idx)
    worst = cr.check_gradients("caffe C = %d, B = %d:" % (C, B), got, loss, g64, l64, e32, el32)
    print("caffe C = %d, B = %d: largest ratio %.2f" % (C, B, worst))
    assert all(np.abs(g64[k]).max() > 0 for k in g64)
    assert loss == loss2 and _same(got, again)


# ---- 2. nothing is clamped -----------------------------------------------------------------------------------------------------

def test_nothing_is_clamped():
    """Both conv biases at -4: every pooled value of both convolutions is negative.  The Caffe network passes all of them on
    and routes every gradient back; Net clamps all of them, and its convolution weights get exactly zero."""
    from gpd_amd import api
    C, B = 3, 5
    img, lab = cr.images(C), cr.labels()
    st = {k: np.array(v) for k, v in cr.xavier_state(C).items()}
    st["conv1.bias"][:] = -4
    st["conv2.bias"][:] = -4
    idx = _batch(B)
    g64, l64, e32, el32 = cr.yardstick(st, img[idx], lab[idx])
    assert np.abs(g64["conv1.weight"]).max() > 0 and np.abs(g64["conv2.weight"]).max() > 0  # a condition on the reference alone
    with _Rig(C) as t:
        t.set_state(st)
        t.set_data(img, lab)
        got, loss = t.gradients(idx)
    cr.check_gradients("caffe, conv biases -4:", got, loss, g64, l64, e32, el32)
    assert np.abs(got["conv1.weight"]).max() > 0 and np.abs(got["conv2.weight"]).max() > 0
    with _Rig(C, recipe=None) as t:
        t.set_state(st)
        t.set_data(img, lab)
        net, _ = t.gradients(idx)
    assert not net["conv1.weight"].any() and not net["conv2.weight"].any()
    # and the recipe's two halves are independent: Net under SGD still clamps
    with _Rig(C, recipe=api.train_default_recipe(1, network=api.NET_TORCH)) as t:
        t.set_state(st)
        t.set_data(img, lab)
        net_sgd, _ = t.gradients(idx)
    assert _same(net, net_sgd)


# ---- 3. ties -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", [0, 200])
def test_every_window_ties(value):
    """All-zero and constant images: every pooling window of conv1 ties (and of conv2, where pool1 is constant per channel),
    with negative pooled values among them (odd biases are -0.1): the gradient hangs on routing to the FIRST maximum."""
    C, B = 1, 5
    img = np.full((B, 60, 60, C), value, np.uint8)
    lab = np.array([0, 1, 1, 0, 1], np.uint8)
    st = cr.xavier_state(C)
    g64, l64, e32, el32 = cr.yardstick(st, img, lab)
    with _Rig(C) as t:
        t.set_state(st)
        t.set_data(img, lab)
        got, loss = t.gradients(np.arange(B, dtype=np.int32))
    cr.check_gradients("caffe constant %d:" % value, got, loss, g64, l64, e32, el32)
    if value == 0:
        assert not got["conv1.weight"].any()
    assert np.abs(got["conv1.bias"]).max() > 0 and np.abs(got["conv2.weight"]).max() > 0


# ---- 4, 5. the SGD rule, its schedule and its multipliers ----------------------------------------------------------------------

N_SET = 20
ROWS = np.array([np.random.RandomState(40 + r).permutation(N_SET)[:5] for r in range(6)], np.int32)  # no image twice in a row
STEP_HYPER = dict(lr_policy="step", stepsize=2, gamma=0.5, momentum=0.5, weight_decay=0.0)
FROZEN = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "fc2.weight", "fc2.bias")
BIASES = ("conv1.bias", "conv2.bias", "fc1.bias", "fc2.bias")
CASES = {"solver file": ({}, None, None), "step": (STEP_HYPER, None, None),
         "frozen": ({}, dict.fromkeys(FROZEN, 0.0), None), "no bias decay": ({}, None, dict.fromkeys(BIASES, 0.0))}


def _sgd_steps(C, hyper, lr_mult=None, decay_mult=None, rows=ROWS, calls="one"):
    recipe, kw = cr.recipe(hyper, lr_mult, decay_mult)
    with _Rig(C, recipe=recipe, **kw) as t:
        t.set_state(cr.xavier_state(C))
        t.set_data(cr.images(C)[:N_SET], cr.labels()[:N_SET])
        losses = t.steps(rows) if calls == "one" else np.concatenate([t.steps(r[None, :]) for r in rows])
        return losses, t.get_state()


@pytest.mark.parametrize("case", list(CASES))
def test_sgd_trajectory_against_the_caffe_rule(case):
    from gpd_amd import api
    C = 3
    hyper, lr_mult, decay_mult = CASES[case]
    st0, lab = cr.xavier_state(C), cr.labels()[:N_SET]
    assert len({tuple(lab[r].tolist()) for r in ROWS}) == len(ROWS)  # the labels differ from row to row: a wrong row shows
    l64, s64, el32, e32 = cr.sgd_trajectory_yardstick(st0, cr.images(C)[:N_SET], lab, ROWS, hyper, lr_mult, decay_mult)
    losses, state = _sgd_steps(C, hyper, lr_mult, decay_mult)
    assert losses.shape == (len(ROWS),) and losses.dtype == np.float32
    bad = []
    for s in range(len(ROWS)):
        err, allow = abs(float(losses[s]) - l64[s]), max(cr.FACTOR * el32[s], 2.0 ** -21)
        print("%s step %d: loss f64 %.9g  device %.9g  e32 = %.3g  error = %.3g  allowance = %.3g" % (case, s, l64[s], losses[s], el32[s], err, allow))
        if err > allow:
            bad.append((s, err, allow))
    for k in api.TORCH_KEYS:
        err = float(np.abs(state[k].astype(np.float64) - s64[k]).max())
        allow = max(cr.FACTOR * e32[k], float(np.spacing(np.float32(np.abs(s64[k]).max()))))
        moved = float(np.abs(s64[k] - st0[k]).max())
        print("%s %-12s e32 = %.3g  device error = %.3g  ratio = %.2f  allowance = %.3g  moved by %.3g" % (case, k, e32[k], err, err / e32[k] if e32[k] else 0.0, allow, moved))
        if err > allow:
            bad.append((k, err, allow))
        if lr_mult and k in lr_mult:
            assert state[k].tobytes() == st0[k].tobytes(), k  # frozen: the same bytes
            assert moved == 0
        else:
            assert moved > 1e-5, (k, moved)
    assert not bad, bad


def test_the_schedule_and_the_multipliers_matter():
    """The references of the four cases differ from one another by far more than their allowances: a device that ignored the
    policy, the momentum or a multiplier could not pass them all (float64 on the CPU; no device in this test)."""
    import torch
    C = 3
    st0, img, lab = cr.xavier_state(C), cr.images(C)[:N_SET], cr.labels()[:N_SET]
    base = cr.sgd_trajectory(st0, img, lab, ROWS, torch.float64)[1]
    fixed = cr.sgd_trajectory(st0, img, lab, ROWS, torch.float64, dict(lr_policy="fixed"))[1]
    nodecay = cr.sgd_trajectory(st0, img, lab, ROWS, torch.float64, None, None, dict.fromkeys(BIASES, 0.0))[1]
    assert np.abs(base["fc1.weight"] - fixed["fc1.weight"]).max() > 1e-7
    assert np.abs(base["fc1.bias"] - nodecay["fc1.bias"]).max() > 1e-7


# ---- 6. the counter ------------------------------------------------------------------------------------------------------------

ROWS12 = np.array([np.random.RandomState(40 + r).permutation(N_SET)[:5] for r in range(12)], np.int32)


def test_counter_and_reproducibility():
    C = 3
    one = _sgd_steps(C, {}, rows=ROWS12)
    again = _sgd_steps(C, {}, rows=ROWS12)
    twelve = _sgd_steps(C, {}, rows=ROWS12, calls="twelve")
    for other in (again, twelve):
        assert one[0].tobytes() == other[0].tobytes() and _same(one[1], other[1])
    # the schedule is in those bytes: a counter that stood still is the fixed policy, and that gives other bytes
    fixed = _sgd_steps(C, dict(lr_policy="fixed"), rows=ROWS12)
    assert not _same(one[1], fixed[1])
    # set_state restarts the schedule (and clears the history): the same twelve steps again, in the same trainer
    recipe, kw = cr.recipe({})
    with _Rig(C, recipe=recipe, **kw) as t:
        t.set_data(cr.images(C)[:N_SET], cr.labels()[:N_SET])
        t.set_state(cr.xavier_state(C))
        t.steps(ROWS12[:7])
        assert t.get_solver_state()["count"] == 7
        t.set_state(cr.xavier_state(C))
        s = t.get_solver_state()
        assert s["count"] == 0 and not any(v.any() for v in s["m"].values()) and s["v"] is None
        losses = t.steps(ROWS12)
        assert losses.tobytes() == one[0].tobytes() and _same(t.get_state(), one[1])
        assert t.get_solver_state()["count"] == 12


# ---- 7. resume -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("solver", ["sgd", "adam"])
def test_resume_continues_byte_for_byte(solver):
    from gpd_amd import api
    C = 3
    img, lab = cr.images(C)[:N_SET], cr.labels()[:N_SET]
    if solver == "sgd":
        recipe, kw = cr.recipe({})
    else:
        recipe, kw = None, {}

    def start():
        rig = _Rig(C, recipe=recipe, **kw)
        rig.trainer.set_data(img, lab)
        return rig

    with start() as t:
        t.set_state(cr.xavier_state(C))
        whole = t.steps(ROWS)
        want, want_solver = t.get_state(), t.get_solver_state()
    with start() as t:
        t.set_state(cr.xavier_state(C))
        first = t.steps(ROWS[:3])
        state, solver_state = t.get_state(), t.get_solver_state()
    assert solver_state["count"] == 3 and (solver_state["v"] is None) == (solver == "sgd")
    assert any(v.any() for v in solver_state["m"].values())
    with start() as t:
        t.set_state(state)
        forgot = t.steps(ROWS[3:])  # without the solver state the run is another one
        forgotten = t.get_state()
        t.set_state(state)
        t.set_solver_state(solver_state)
        second = t.steps(ROWS[3:])
        got, got_solver = t.get_state(), t.get_solver_state()
        # refused, and nothing changed: a non-finite value, a missing buffer, a negative count
        broken = dict(solver_state, m={k: v.copy() for k, v in solver_state["m"].items()})
        broken["m"]["fc1.weight"][3, 5] = np.nan
        with pytest.raises(api.GpdHipError, match="non-finite"):
            t.set_solver_state(broken)
        with pytest.raises(api.GpdHipError):
            t.set_solver_state(dict(solver_state, count=-1))
        if solver == "adam":
            with pytest.raises(api.GpdHipError):
                t.set_solver_state(dict(solver_state, v=None))
        after = t.get_solver_state()
    assert np.concatenate([first, second]).tobytes() == whole.tobytes()
    assert _same(got, want) and got_solver["count"] == want_solver["count"] == 6
    assert _same(got_solver["m"], want_solver["m"]) and (solver == "sgd" or _same(got_solver["v"], want_solver["v"]))
    assert not _same(forgotten, want) and forgot.tobytes() != second.tobytes()
    assert after["count"] == 6 and _same(after["m"], got_solver["m"])


# ---- 8. eval -------------------------------------------------------------------------------------------------------------------

def test_eval_of_the_caffe_network():
    C, n = 3, 70
    img, lab, st = cr.images(C), cr.labels(), cr.xavier_state(C)
    z64, e32, _ = cr.logits_yardstick(st, img)
    want_correct = int(((z64[:, 1] > z64[:, 0]) == (lab == 1)).sum())
    with _Rig(C, max_batch=64) as t:
        t.set_state(st)
        t.set_data(img[:8], lab[:8])
        t.set_data(img[::-1], lab[::-1], which=1)   # the test slot holds the set back to front
        logits, correct = t.eval(n=n, which=1)      # chunks of 64 + 6
        short, _ = t.eval(np.array([69 - 5], np.int32), which=1)
    err = float(np.abs(logits - z64[::-1]).max())
    print("caffe eval: |logits - f64| = %.3g, float32 forward error %.3g, ratio %.2f, %d correct (float64: %d)" % (err, e32, err / e32, correct, want_correct))
    assert logits.shape == (n, 2) and logits.dtype == np.float32
    assert err <= 4 * e32
    assert correct == want_correct and 0 < want_correct < n
    assert short[0].tobytes() == logits[64].tobytes()  # image 5 is the first of the short chunk: the same bytes alone


# ---- 9. into scoring -----------------------------------------------------------------------------------------------------------

def test_round_trip_into_scoring(tmp_path):
    from gpd_amd import api, eigen_export
    C = 3
    img = cr.images(C)
    losses, state = _sgd_steps(C, {})
    z64, _, _ = cr.logits_yardstick(state, img)
    d64 = z64[:, 1] - z64[:, 0]
    eigen_export.export(state, str(tmp_path / "params"), 1.0 / 256)
    w = eigen_export.load(str(tmp_path / "params"))
    recipe, kw = cr.recipe({})
    with _Rig(C, recipe=recipe, **kw) as t:
        ctx = t._ctx
        t.set_state(state)
        scores = {}
        for mode in (api.LENET_SPLIT, api.LENET_F32_CHAIN):
            ctx.set_lenet_mode(mode)
            ctx.set_lenet_conv_relu(False)
            ctx.set_lenet_weights(w)
            sc = ctx.score(img)
            err = float(np.abs(sc - d64).max())
            print("caffe round trip, mode %d: max |score - f64| = %.3g, max |score| = %.3g" % (mode, err, float(np.abs(d64).max())))
            assert sc.shape == (70,) and err <= 1e-4, (mode, err)
            ctx.set_lenet_conv_relu(True)   # install has to switch it off again
            t.install(ctx)
            assert np.array_equal(ctx.score(img), sc), mode
            scores[mode] = sc
        ctx.set_lenet_conv_relu(True)       # ... and the flag does matter to these weights
        assert np.abs(ctx.score(img) - scores[api.LENET_F32_CHAIN]).max() > 1e-3
    with _Rig(C, recipe=None) as t:         # Net's install still switches it on
        t.set_state(state)
        t._ctx.set_lenet_mode(api.LENET_F32_CHAIN)
        t.install()
        assert np.abs(t._ctx.score(img) - scores[api.LENET_F32_CHAIN]).max() > 1e-3


# ---- 10. the existing recipe -----------------------------------------------------------------------------------------------------

def test_the_default_recipe_is_the_trainer_without_one():
    from gpd_amd import api
    C = 3
    img, lab = cr.images(C)[:N_SET], cr.labels()[:N_SET]
    out = []
    for recipe in (None, api.train_default_recipe(0)):
        with _Rig(C, recipe=recipe) as t:
            t.set_state(api.init_state(C, 1))
            t.set_data(img, lab)
            losses = t.steps(ROWS[:3])
            out.append((losses, t.get_state(), t.get_solver_state(), [n for n, _ in t.step_timed(ROWS[0])]))
    assert out[0][0].tobytes() == out[1][0].tobytes() and _same(out[0][1], out[1][1])
    assert _same(out[0][2]["m"], out[1][2]["m"]) and _same(out[0][2]["v"], out[1][2]["v"]) and out[0][2]["count"] == out[1][2]["count"] == 3
    assert out[0][3] == out[1][3] and out[0][3][-1] == "adam"
    with _Rig(C) as t:
        t.set_state(cr.xavier_state(C))
        t.set_data(img, lab)
        names = [n for n, _ in t.step_timed(ROWS[0])]
    assert names == out[0][3][:-1] + ["sgd"]
    # multipliers are the SGD solver's
    with pytest.raises(api.GpdHipError, match="recipe"):
        _Rig(C, recipe=api.train_default_recipe(0, lr_mult={"conv1.weight": 0.0}))


# ---- 11. the tool ----------------------------------------------------------------------------------------------------------------

def test_the_tool_trains_the_caffe_recipe_and_detect_grasps_loads_it(tmp_path):
    import train_ref as tr
    from gpd_amd import api, eigen_export, synth
    from test_host_cli import CLI, _subsample_indices, _write_case
    C, S, K = 3, 30, 10
    img, lab, _ = tr.learn_set(C)
    data = tmp_path / "data"
    data.mkdir()
    for prefix in ("train", "test"):
        np.save(str(data / (prefix + "_images.npy")), img)
        np.save(str(data / (prefix + "_labels.npy")), lab)
    cl = synth.make_cloud(5, 2000)
    cfg, pcd = _write_case(tmp_path, cl, synth.lenet_weights(C), S, K, channels=C)
    params = tmp_path / "params"
    for f in os.listdir(str(params)):  # what _write_case put there: the tool writes this directory
        os.remove(str(params / f))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "gpd_amd.train", str(data), "--test", str(data), "--recipe", "caffe", "--max-iter", "200", "--seed", "1"]
    run = subprocess.run(base + ["--snapshot", "100", "--out", str(params)], capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=300)
    print(run.stdout[-3000:])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = [l for l in run.stdout.splitlines() if l.startswith("Iteration ")]
    assert [l.split(",")[0] for l in lines] == ["Iteration 100", "Iteration 200"] and all("lr = " in l and "loss = " in l and "accuracy = " in l for l in lines)
    assert ("lr = %.6g" % float(api.learning_rate(api.train_default_recipe(1), 0.01, 199))) in lines[1]
    names = sorted(eigen_export.FILES.values())
    assert sorted(f for f in os.listdir(str(params)) if f.endswith(".bin")) == names and not (params / "network.cfg").exists()
    # --resume from the snapshot at 100 ends in the same bytes
    again = tmp_path / "again"
    run2 = subprocess.run(base + ["--resume", str(params / "snapshot_100"), "--out", str(again)], capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=300)
    assert run2.returncode == 0, run2.stdout[-2000:] + run2.stderr[-2000:]
    for name in names:
        assert (params / name).read_bytes() == (again / name).read_bytes(), name
    # the directory is a weights_file: detect_grasps prints the scores of the Python path on the same files
    out = subprocess.run([CLI, str(cfg), str(pcd)], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = np.array([float(l.split()[1]) for l in out.stdout.splitlines() if l.startswith("GRASP ")], np.float32)
    ctx = api.Context(api.default_params(C))
    try:
        ctx.set_lenet_weights(eigen_export.load(str(params)))
        ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
        sel, _, n_cand = ctx.detect_select(_subsample_indices(len(cl["xyz"]), S), K)
        assert len(sel) == K and n_cand > K
        assert np.array_equal(got, sel["score"])
        acc = float(((ctx.score(img) > 0) == (lab == 1)).mean())
    finally:
        ctx.close()
    print("the trained network scores its set with accuracy %.4f" % acc)
    assert acc >= 0.95


def test_the_tool_fits_ip1_under_given_convolutions(tmp_path):
    """--init DIR --freeze conv1,conv2,fc2 on a directory without ip1_weights.bin (the reference's snapshot): the six frozen
    tensors come out as the bytes that went in, ip1 starts from the xavier filler and moves."""
    import train_ref as tr
    from gpd_amd import api, eigen_export, train
    C = 3
    img, lab, _ = tr.learn_set(C)
    data, given, out = tmp_path / "data", tmp_path / "given", tmp_path / "out"
    data.mkdir()
    np.save(str(data / "train_images.npy"), img)
    np.save(str(data / "train_labels.npy"), lab)
    eigen_export.export(cr.xavier_state(C, seed=9), str(given))
    os.remove(str(given / "ip1_weights.bin"))
    assert train.main([str(data), "--recipe", "caffe", "--max-iter", "3", "--seed", "4", "--init", str(given), "--freeze", "conv1,conv2,fc2",
                       "--out", str(out)]) == 0
    for name in sorted(eigen_export.FILES.values()):
        if name.startswith("ip1"):
            continue
        assert (out / name).read_bytes() == (given / name).read_bytes(), name
    start = api.lenet_from_torch(api.init_xavier(C, 4), C)["f1w"]
    got = np.fromfile(str(out / "ip1_weights.bin"), "<f4")
    moved = np.abs(got - start).max()
    print("ip1 moved by %.3g in three iterations" % moved)
    assert got.size == start.size and 0 < moved < 0.1  # three steps of lr 0.01 on weights below 0.021
    assert (out / "ip1_biases.bin").read_bytes() != (given / "ip1_biases.bin").read_bytes()
