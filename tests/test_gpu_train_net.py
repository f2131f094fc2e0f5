"""Trainers of any network of the family (gpd_hip_train_create_net): other widths and NetCCFFF's third dense
layer, against float64 autograd and torch.optim.Adam (train_net_ref), against the composed route, and through the tool.
max_batch is the batch used everywhere, to keep the allocations small."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import train_net_ref as nr
import train_ref as tr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Rig:
    """A context and a trainer on it, closed in order."""

    def __init__(self, C_, **kw):
        from gpd_amd import api
        self.ctx = api.Context(api.default_params(C_))
        try:
            self.trainer = api.Trainer(self.ctx, api.train_default_params(C_, kw.pop("max_batch", 64)), kw.pop("recipe", None), **kw)
        except Exception:
            self.ctx.close()
            raise

    def __enter__(self):
        return self.trainer

    def __exit__(self, *exc):
        self.trainer.close()
        self.ctx.close()


def _same(a, b):
    return set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)


def _same_solver(a, b):
    return a["count"] == b["count"] and _same(a["m"], b["m"]) and ((a["v"] is None and b["v"] is None) or _same(a["v"], b["v"]))


def _recipe(solver):
    """-> (recipe or None, lr): "adam" — the default recipe; "sgd" — the Caffe recipe (the network without conv ReLUs, SGD)"""
    from gpd_amd import api
    return (None, 1e-3) if solver == "adam" else (api.train_default_recipe(1), api.CAFFE_BASE_LR)


# ---- 1. gradients ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims,B,caffe", [((1, 1, 1, 1, 0), 1, False), ((3, 33, 65, 31, 0), 5, False), ((15, 6, 16, 120, 84), 5, False),
                                          ((15, 6, 16, 120, 84), 64, False), ((12, 10, 20, 100, 33), 3, False), ((12, 10, 20, 100, 33), 3, True),
                                          ((1, 64, 128, 1024, 1024), 2, False)])
def test_gradients_against_float64_autograd(dims, B, caffe):
    from gpd_amd import api
    Cn = dims[0]
    img, lab = tr.images(Cn), tr.labels()
    st = api.init_state(Cn, 2, shape=dims[1:])
    idx = (len(lab) - 1 - np.arange(B)).astype(np.int32)
    idx[: B // 2] = idx[: B // 2][::-1]
    g64, l64, e32, el32 = nr.yardstick(st, img[idx], lab[idx], conv_relu=not caffe)
    assert all(np.abs(g).max() > 0 for g in g64.values())  # the inputs reach every tensor, at one unit per layer too (seed 2)
    recipe = api.train_default_recipe(0, network=api.NET_CAFFE) if caffe else None
    with _Rig(Cn, max_batch=B, recipe=recipe, shape=dims[1:]) as t:
        assert t.shape.as_tuple() == dims
        t.set_state(st)
        t.set_data(img, lab)
        got, loss = t.gradients(idx)
        again, loss2 = t.gradients(idx)
    what = "%s%s, B = %d:" % (dims, " (no conv ReLU)" if caffe else "", B)
    worst = nr.check_gradients(what, got, loss, g64, l64, e32, el32)
    print("%s largest ratio %.2f" % (what, worst))
    assert loss == loss2 and _same(got, again)


# ---- 2. the stock shape through create_net -------------------------------------------------------------------------------------

@pytest.mark.parametrize("solver", ["adam", "sgd"])
def test_stock_shape_is_the_stock_trainer(solver):
    from gpd_amd import api
    Cn, B = 3, 5
    img, lab = tr.images(Cn), tr.labels()
    rows = np.arange(3 * B, dtype=np.int32).reshape(3, B)
    recipe, lr = _recipe(solver)
    out = []
    for shape in (None, (20, 50, 500), (20, 50, 500, 0)):
        with _Rig(Cn, max_batch=B, recipe=recipe, shape=shape, lr=lr) as t:
            t.set_data(img, lab)
            t.set_state(api.init_state(Cn, 1))
            losses = t.steps(rows)
            out.append((losses, t.get_state(), t.get_solver_state()))
            assert [n for n, _ in t.step_timed(rows[0])][-1] == solver
    for losses, state, solver_state in out[1:]:
        assert losses.tobytes() == out[0][0].tobytes()
        assert _same(state, out[0][1]) and _same_solver(solver_state, out[0][2])
    assert np.isfinite(out[0][0]).all() and out[0][2]["count"] == 3


# ---- 3. steps == gradients + apply -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(3, 33, 65, 31, 0), (15, 6, 16, 120, 84)])
@pytest.mark.parametrize("solver", ["adam", "sgd"])
def test_steps_are_gradients_and_apply(dims, solver):
    from gpd_amd import api
    Cn, B = dims[0], 5
    img, lab = tr.images(Cn), tr.labels()
    rows = (np.arange(3 * B, dtype=np.int32).reshape(3, B) * 3) % len(lab)
    recipe, lr = _recipe(solver)
    st = api.init_state(Cn, 2, shape=dims[1:])
    with _Rig(Cn, max_batch=B, recipe=recipe, shape=dims[1:], lr=lr) as t:
        t.set_data(img, lab)
        t.set_state(st)
        losses = t.steps(rows)
        a, sa = t.get_state(), t.get_solver_state()
        t.set_state(st)
        composed = []
        for row in rows:
            g, loss = t.gradients(row)
            t.apply(g)
            composed.append(loss)
        b, sb = t.get_state(), t.get_solver_state()
    assert losses.tobytes() == np.array(composed, np.float32).tobytes()
    assert _same(a, b) and _same_solver(sa, sb)
    assert any(not np.array_equal(a[k], st[k]) for k in a)


# ---- 4. Adam against torch -------------------------------------------------------------------------------------------------------

def test_adam_trajectory_against_torch():
    from gpd_amd import api
    dims, B = (15, 6, 16, 120, 84), 5
    img, lab = tr.images(15), tr.labels()
    rows = (np.arange(3 * B, dtype=np.int32).reshape(3, B) * 7) % len(lab)
    st = api.init_state(15, 4, shape=dims[1:])
    l64, s64, el32, e32 = nr.trajectory_yardstick(st, img, lab, rows)
    with _Rig(15, max_batch=B, shape=dims[1:]) as t:
        t.set_data(img, lab)
        t.set_state(st)
        losses = t.steps(rows)
        got = t.get_state()
    bad = []
    for s in range(3):
        err, allow = abs(float(losses[s]) - l64[s]), max(nr.FACTOR * el32[s], 2.0 ** -21)
        print("step %d loss: f64 %.9g  device %.9g  error %.3g  allowance %.3g" % (s, l64[s], losses[s], err, allow))
        if err > allow:
            bad.append(("loss", s, err, allow))
    for k in s64:
        err = float(np.abs(got[k].astype(np.float64) - s64[k]).max())
        allow = max(nr.FACTOR * e32[k], float(np.spacing(np.float32(np.abs(s64[k]).max()))))
        print("Adam %-12s torch f32 error %.3g  device error %.3g  allowance %.3g  moved by %.3g" % (k, e32[k], err, allow, float(np.abs(s64[k] - st[k]).max())))
        if err > allow:
            bad.append((k, err, allow))
    assert not bad, bad


# ---- 5. snapshot -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("solver", ["adam", "sgd"])
def test_a_snapshot_continues_to_the_bit(solver):
    from gpd_amd import api
    dims, B = (3, 6, 16, 120, 84), 5
    img, lab = tr.images(3), tr.labels()
    rows = (np.arange(4 * B, dtype=np.int32).reshape(4, B) * 3) % len(lab)
    recipe, lr = _recipe(solver)
    st = api.init_state(3, 6, shape=dims[1:])
    with _Rig(3, max_batch=B, recipe=recipe, shape=dims[1:], lr=lr) as t:
        t.set_data(img, lab)
        t.set_state(st)
        whole = t.steps(rows)
        end, end_solver = t.get_state(), t.get_solver_state()
        t.set_state(st)
        first = t.steps(rows[:2])
        snap, snap_solver = t.get_state(), t.get_solver_state()
    with _Rig(3, max_batch=B, recipe=recipe, shape=dims[1:], lr=lr) as t:
        t.set_data(img, lab)
        t.set_state(snap)
        t.set_solver_state(snap_solver)
        rest = t.steps(rows[2:])
        assert np.concatenate([first, rest]).tobytes() == whole.tobytes()
        assert _same(t.get_state(), end) and _same_solver(t.get_solver_state(), end_solver)
    assert snap_solver["count"] == 2 and len(snap) == 10


# ---- 6. it learns, and the loop closes ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _trained():
    from gpd_amd import api
    img, lab, idx = tr.learn_set(3)
    st0 = api.init_state(3, 1, shape=(6, 16, 120, 84))
    with _Rig(3, max_batch=64, shape=(6, 16, 120, 84)) as t:
        t.set_state(st0)
        t.set_data(img, lab)
        losses = t.steps(idx)
        logits, correct = t.eval(n=256)
        ctx = t._ctx
        t.install(ctx)
        info = ctx.lenet_net_info()
        score = ctx.score(img)
        return dict(state0=st0, state=t.get_state(), losses=losses, logits=logits, correct=correct, info=info, score=score)


def test_it_learns():
    """(3; 6, 16, 120, 84) on train_ref.learn_set(3), 40 steps from init_state(3, 1, shape).  torch in float64 over the same 40
    rows (train_net_ref.trajectory) goes from a loss of 0.691232 to 5.2e-06 and reaches a training accuracy of 1.0 (256 of
    256) after these 40 steps, so no further epochs were needed; the device must reach 1.0 - 5/256."""
    import torch
    img, lab, idx = tr.learn_set(3)
    r = _trained()
    losses, acc = r["losses"], r["correct"] / 256.0
    print("loss %.6g -> %.6g, training accuracy %.4f (torch float64: 1.0)" % (losses[0], losses[-1], acc))
    assert losses.shape == (40,) and np.isfinite(losses).all()
    z = nr.logits(r["state0"], img[idx[0]], torch.float64)
    s = z[:, 1] - z[:, 0]
    want = float(np.log1p(np.exp(np.where(lab[idx[0]] == 1, -s, s))).mean())
    print("first loss %.9g, float64 %.9g" % (losses[0], want))
    assert abs(float(losses[0]) - want) <= 2.0 ** -20
    assert losses[-1] < losses[0]
    assert acc >= 1.0 - 5.0 / 256
    assert r["correct"] == int(((r["logits"][:, 1] > r["logits"][:, 0]) == (lab == 1)).sum())


def test_the_loop_closes():
    """Trainer.install puts the trained NetCCFFF onto the context's general route (lenet_net_info succeeds there only), whose
    score and eval's logit1 - logit0 are two float32 summation orders of one network: 4 e32 apart at the most, e32 from torch's
    two float32 forwards against float64 as in test_gpu_train.test_the_loop_closes."""
    import torch
    img, lab, _ = tr.learn_set(3)
    r = _trained()
    assert r["info"]["chunk_images"] > 0 and r["info"]["macs_per_image"] > 0
    truth = nr.logits(r["state"], img, torch.float64)
    t64 = truth[:, 1] - truth[:, 0]
    a = nr.logits(r["state"], img, torch.float32)
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        b = nr.logits(r["state"], img[::-1], torch.float32)[::-1]
    finally:
        torch.set_num_threads(before)
    e32 = max(float(np.abs((a[:, 1] - a[:, 0]) - t64).max()), float(np.abs((b[:, 1] - b[:, 0]) - t64).max()))
    dev = r["logits"][:, 1] - r["logits"][:, 0]
    err = float(np.abs(r["score"].astype(np.float64) - dev).max())
    print("|score - (logit1 - logit0)| = %.3g, e32 = %.3g, ratio %.2f; |eval - f64| = %.3g" % (err, e32, err / e32, float(np.abs(dev - t64).max())))
    assert err <= 4 * e32


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_trainer_usable():
    from gpd_amd import api
    L = api.lib()
    Cn, B = 3, 4
    img, lab = tr.images(Cn), tr.labels()
    ctx = api.Context(api.default_params(Cn))
    ctx2 = api.Context(api.default_params(Cn))
    try:
        p = api.train_default_params(Cn, B)
        h = C.c_void_p()
        # creation: a shape outside the limits, a channel mismatch, multipliers with a third dense layer
        for dims in ((3, 65, 16, 120, 84), (3, 6, 129, 120, 0), (3, 6, 16, 1025, 0), (3, 6, 16, 120, 1025), (3, 0, 16, 120, 0)):
            assert L.gpd_hip_train_create_net(ctx._h, C.byref(p), None, C.byref(api.LenetShape(*dims)), C.byref(h)) == -1 and not h
            assert b"limits" in L.gpd_hip_last_error()
        assert L.gpd_hip_train_create_net(ctx._h, C.byref(p), None, C.byref(api.LenetShape(15, 6, 16, 120, 84)), C.byref(h)) == -1 and not h
        assert b"channels" in L.gpd_hip_last_error()
        assert L.gpd_hip_train_create_net(ctx._h, C.byref(p), None, None, C.byref(h)) == -1 and not h
        frozen = api.train_default_recipe(1, lr_mult={"conv1.weight": 0.0})
        assert L.gpd_hip_train_create_net(ctx._h, C.byref(p), C.byref(frozen), C.byref(api.LenetShape(3, 6, 16, 120, 84)), C.byref(h)) == -1 and not h
        assert b"multiplier" in L.gpd_hip_last_error()
        decayed = api.train_default_recipe(1, decay_mult={"fc2.bias": 0.0})
        with pytest.raises(api.GpdHipError):
            api.Trainer(ctx, p, decayed, shape=(6, 16, 120, 84))
        # ... which two dense layers take at any widths
        api.Trainer(ctx, api.train_default_params(Cn, B), frozen, shape=(6, 16, 120)).close()

        t = api.Trainer(ctx, p, shape=(6, 16, 120, 84))
        st = api.init_state(Cn, 9, shape=(6, 16, 120, 84))
        t.set_data(img, lab)
        t.set_state(st)
        idx = np.arange(B, dtype=np.int32)
        want, want_loss = t.gradients(idx)
        # the entries with tables of 8 on a trainer of ten tensors: GPD_ERR_STATE, nothing changed
        bufs = [np.full(s, 7.0, np.float32) for s in api.net_state_shapes(t.shape)[:8]]
        t8 = (C.c_void_p * 8)(*[b.ctypes.data for b in bufs])
        n, loss = C.c_longlong(-5), C.c_float(-5)
        assert L.gpd_hip_train_get_state(t._h, t8) == -4
        assert L.gpd_hip_train_set_state(t._h, t8) == -4
        assert L.gpd_hip_train_gradients(t._h, idx.ctypes.data, B, t8, C.byref(loss)) == -4
        assert L.gpd_hip_train_apply(t._h, t8) == -4
        assert L.gpd_hip_train_get_solver_state(t._h, t8, t8, C.byref(n)) == -4
        assert L.gpd_hip_train_set_solver_state(t._h, t8, t8, 3) == -4
        assert all((b == 7.0).all() for b in bufs) and n.value == -5 and loss.value == -5
        assert _same(t.get_state(), st) and t.get_solver_state()["count"] == 0
        # a table of 10 with a NULL among its used slots
        arrs, ptrs = api._net_pointers(st, t.shape)
        for slot in (0, 8, 9):
            broken = (C.c_void_p * 10)(*[None if i == slot else a.ctypes.data for i, a in enumerate(arrs)])
            assert L.gpd_hip_train_net_set_state(t._h, broken) == -1
            assert L.gpd_hip_train_net_get_state(t._h, broken) == -1
            assert L.gpd_hip_train_net_apply(t._h, broken) == -1
            assert L.gpd_hip_train_net_gradients(t._h, idx.ctypes.data, B, broken, C.byref(loss)) == -1
            assert L.gpd_hip_train_net_set_solver_state(t._h, broken, broken, 0) == -1
            assert L.gpd_hip_train_net_get_solver_state(t._h, broken, broken, C.byref(n)) == -1
        assert _same(t.get_state(), st) and t.get_solver_state()["count"] == 0
        # a group of two shapes
        other = api.Trainer(ctx2, api.train_default_params(Cn, B), shape=(6, 16, 120))
        with pytest.raises(api.GpdHipError):
            api.TrainerGroup([t, other])
        other.close()
        # after all of it the trainer computes what it computed
        again, again_loss = t.gradients(idx)
        assert again_loss == want_loss and _same(again, want)
        assert np.isfinite(t.steps(idx[None, :])).all()
        # a trainer of two dense layers takes both tables, slots [8] and [9] NULL
        t6 = api.Trainer(ctx2, api.train_default_params(Cn, B), shape=(6, 16, 120))
        st6 = api.init_state(Cn, 9, shape=(6, 16, 120))
        t6.set_state(st6)
        out8 = [np.zeros(s, np.float32) for s in api.net_state_shapes(t6.shape)]
        assert L.gpd_hip_train_get_state(t6._h, (C.c_void_p * 8)(*[b.ctypes.data for b in out8])) == 0
        assert all(o.tobytes() == st6[k].tobytes() for o, k in zip(out8, api.TORCH_KEYS))
        t6.close()
        t.close()
    finally:
        ctx2.close()
        ctx.close()


# ---- 8. group ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("solver", ["adam", "sgd"])
def test_group_of_two_is_the_composed_route(solver):
    from gpd_amd import api
    dims, B, G = (3, 6, 16, 120, 84), 4, 2
    img, lab = tr.images(3), tr.labels()
    rows = np.stack([(np.arange(2 * B, dtype=np.int32).reshape(2, B) * (3 + r) + r) % 35 for r in range(G)])
    recipe, lr = _recipe(solver)
    st = api.init_state(3, 8, shape=dims[1:])
    ctxs = [api.Context(api.default_params(3)) for _ in range(G)]
    ts = []
    try:
        ts = [api.Trainer(c, api.train_default_params(3, B), recipe, shape=dims[1:], lr=lr) for c in ctxs]
        for r, t in enumerate(ts):
            t.set_data(img[r::G], lab[r::G])
        group = api.TrainerGroup(ts)
        ts[0].set_state(st)
        group.broadcast(0)
        losses, each = group.steps(rows)
        assert group.verify() == 0
        got, got_solver = ts[1].get_state(), ts[1].get_solver_state()
        assert sum(a.size for a in got.values()) == sum(api.net_sizes(ts[0].shape))
        group.close()
        # the composed route on the same trainers
        for t in ts:
            t.set_state(st)
        want_losses = []
        for s in range(rows.shape[1]):
            gl = [t.gradients(rows[r, s]) for r, t in enumerate(ts)]
            mean = {k: api.train_group_mean([g[k] for g, _ in gl]) for k in gl[0][0]}
            want_losses.append(api.train_group_mean([np.array([l], np.float32) for _, l in gl])[0])
            for t in ts:
                t.apply(mean)
        assert losses.tobytes() == np.array(want_losses, np.float32).tobytes()
        for t in ts:
            assert _same(t.get_state(), got) and _same_solver(t.get_solver_state(), got_solver)
    finally:
        for t in ts:
            t.close()
        for c in ctxs:
            c.close()


# ---- 9. the tool ---------------------------------------------------------------------------------------------------------------------

def test_command_line_trains_netccfff(tmp_path):
    import torch
    from gpd_amd import api
    rng = np.random.RandomState(3)
    img = rng.randint(0, 256, (16, 60, 60, 3)).astype(np.uint8)
    img[rng.rand(*img.shape) < 0.6] = 0
    data, out = tmp_path / "data", tmp_path / "out"
    data.mkdir()
    np.save(data / "train_images.npy", img)
    np.save(data / "train_labels.npy", rng.randint(0, 2, 16).astype(np.uint8))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gpd_amd.train", str(data), "--net", "6,16,120,84", "--epochs", "1", "--batch", "8", "--out", str(out)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    state = torch.load(str(out / "model.pwf"))
    assert tuple(state) == api.TORCH_NET_KEYS and len(state) == 10
    assert [tuple(v.shape) for v in state.values()] == list(api.net_state_shapes(api.LenetShape(3, 6, 16, 120, 84)))
    for k in api.TORCH_NET_KEYS:
        assert (out / (k + ".bin")).stat().st_size == 4 * state[k].numel()
    assert "fc2_out = 84" in (out / "network.cfg").read_text()
    ctx = api.Context(api.default_params(3))
    try:
        assert ctx.set_lenet_net(state).as_tuple() == (3, 6, 16, 120, 84)
        assert np.isfinite(ctx.score(img)).all()
    finally:
        ctx.close()
