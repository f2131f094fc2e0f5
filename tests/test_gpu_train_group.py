"""gpd_hip_train_group_* (train_group.hip): training on several replicas, held byte for byte to its definition — the
composed route: gradients() on each of G trainers, train_group_mean on the host, apply() on each.

The replicas of every test but the last sit on ONE device, each on a context of its own: the kernels, the copies
(hipMemcpyPeerAsync) and the schedule are the ones that run over several devices.  Data: train_ref.images / labels (70 images).
"""
import functools

import numpy as np
import pytest

import train_ref as tr
from test_gpu_train_edges import ROWS

pytestmark = pytest.mark.gpu

STEPS = 3
# (C, G, batch per replica, recipe)
CASES = [(3, 2, 4, "adam"), (3, 3, 2, "adam"), (1, 2, 3, "caffe"), (15, 2, 2, "adam")]


def _recipe(name):
    """caffe: SGD under the inv policy with eight DIFFERENT multipliers of either kind — the tensors' ends are no multiples of 4
    floats, so a slice or a vector lane that straddles two tensors would show"""
    from gpd_amd import api
    if name == "adam":
        return None
    return api.train_default_recipe(1, lr_mult=[1.0, 2.0, 0.5, 1.5, 0.75, 3.0, 1.25, 0.25], decay_mult=[1.0, 0.0, 2.0, 0.5, 1.5, 0.25, 0.75, 3.0])


def _kw(name):
    from gpd_amd import api
    return dict(recipe=_recipe(name), lr=api.CAFFE_BASE_LR) if name == "caffe" else {}


def _init(C, name):
    from gpd_amd import api
    return api.init_xavier(C, 1) if name == "caffe" else api.init_state(C, 1)


class _Rig:
    """G contexts with a trainer each (replica r on devices[r], default all on device 0), optionally a group; closed in order."""

    def __init__(self, C, G, group=True, devices=None, max_batch=None, **kw):
        from gpd_amd import api
        self.ctxs, self.trainers, self.group = [], [], None
        try:
            for r in range(G):
                self.ctxs.append(api.Context(api.default_params(C), device=devices[r] if devices else 0))
                mb = max_batch[r] if isinstance(max_batch, (list, tuple)) else (max_batch or 8)
                self.trainers.append(api.Trainer(self.ctxs[-1], max_batch=mb, **kw))
            if group:
                self.group = api.TrainerGroup(self.trainers)
        except Exception:
            self.close()
            raise

    def close(self):
        if self.group is not None:
            self.group.close()
        for t in self.trainers:
            t.close()
        for c in self.ctxs:
            c.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _shards(C, G):
    img, lab = tr.images(C), tr.labels()
    return [(img[r::G], lab[r::G]) for r in range(G)]


@functools.lru_cache(maxsize=None)
def _indices(C, G, b, steps=STEPS):
    """i32 [G, steps, b] into the shards img[r::G]; a repeated index is as legal as anywhere"""
    rng = np.random.RandomState(100 * C + 10 * G + b)
    idx = np.stack([rng.randint(0, len(tr.labels()[r::G]), (steps, b)) for r in range(G)]).astype(np.int32)
    idx.setflags(write=False)
    return idx


def _everything(t):
    """A trainer's parameters, solver buffers and count as one comparable dict of bytes"""
    s = t.get_solver_state()
    out = {"p." + k: v.tobytes() for k, v in t.get_state().items()}
    out.update({"m." + k: v.tobytes() for k, v in s["m"].items()})
    if s["v"] is not None:
        out.update({"v." + k: v.tobytes() for k, v in s["v"].items()})
    out["count"] = s["count"]
    return out


@functools.lru_cache(maxsize=None)
def _composed(C, G, b, name):
    """The definition -> (losses f32 [STEPS], each replica's losses f32 [G, STEPS], each replica's _everything)"""
    from gpd_amd import api
    idx = _indices(C, G, b)
    with _Rig(C, G, group=False, **_kw(name)) as rig:
        for t, (img, lab) in zip(rig.trainers, _shards(C, G)):
            t.set_state(_init(C, name))
            t.set_data(img, lab)
        losses, each = [], []
        for s in range(STEPS):
            got = [t.gradients(idx[r, s]) for r, t in enumerate(rig.trainers)]
            mean = {k: api.train_group_mean([g[k] for g, _ in got]) for k in api.TORCH_KEYS}
            for t in rig.trainers:
                t.apply(mean)
            each.append([np.float32(loss) for _, loss in got])
            losses.append(api.train_group_mean([np.array([loss], np.float32) for _, loss in got])[0])
        return np.array(losses, np.float32), np.array(each, np.float32).T.copy(), [_everything(t) for t in rig.trainers]


def _fill(rig, C, G):
    for t, (img, lab) in zip(rig.trainers, _shards(C, G)):
        t.set_data(img, lab)


def _start(rig, C, name):
    """How a group starts: set_state on replica 0, then broadcast"""
    rig.trainers[0].set_state(_init(C, name))
    rig.group.broadcast(0)


def _assert_is_composed(rig, losses, each, case):
    want_losses, want_each, want = _composed(*case)
    assert losses.dtype == np.float32 and losses.tobytes() == want_losses.tobytes(), (case, losses, want_losses)
    assert each.tobytes() == want_each.tobytes(), case
    for r, t in enumerate(rig.trainers):
        got = _everything(t)
        assert got.keys() == want[r].keys()
        for k in got:
            assert got[k] == want[r][k], (case, "replica %d" % r, k)
    assert want[0]["count"] == STEPS and all(w == want[0] for w in want)  # the definition itself keeps the replicas in step
    assert rig.group.verify() == 0


# ---- 1, 9. the composed route, byte for byte -----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=["C3-G2-adam", "C3-G3-adam-uneven", "C1-G2-caffe", "C15-G2-adam"])
def test_equals_the_composed_route(case):
    C, G, b, name = case
    with _Rig(C, G, **_kw(name)) as rig:
        _fill(rig, C, G)
        _start(rig, C, name)
        losses, each = rig.group.steps(_indices(C, G, b))
        _assert_is_composed(rig, losses, each, case)
        moved = rig.trainers[0].get_state()
    st0 = _init(C, name)
    assert all(np.abs(moved[k] - st0[k]).max() > 0 for k in moved)  # every tensor took part


def test_distinct_devices():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("the machine shows one device: transport between distinct devices needs two")
    case = CASES[0]
    C, G, b, name = case
    with _Rig(C, G, devices=[0, 1]) as rig:
        _fill(rig, C, G)
        _start(rig, C, name)
        losses, each = rig.group.steps(_indices(C, G, b))
        _assert_is_composed(rig, losses, each, case)


# ---- 2. one replica ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["adam", "caffe"])
def test_one_replica_is_the_trainer(name):
    C, b = 1, 5
    idx = _indices(C, 1, b)
    with _Rig(C, 1, **_kw(name)) as rig:
        _fill(rig, C, 1)
        _start(rig, C, name)
        losses, each = rig.group.steps(idx)
        got = _everything(rig.trainers[0])
        assert rig.group.verify() == 0 and rig.group.last_bytes()[0] == 0
        t = rig.trainers[0]
        t.set_state(_init(C, name))
        want_losses = t.steps(idx[0])
        want = _everything(t)
    assert losses.tobytes() == want_losses.tobytes() and each.tobytes() == want_losses.tobytes()
    assert got == want and want["count"] == STEPS


# ---- 3. it is large-batch training ----------------------------------------------------------------------------------------------

def test_two_halves_are_one_batch():
    """Both replicas hold all 70 images and take 4 + 4 of each of test_gpu_train_edges.ROWS' rows of 8: the mean of the two
    half-batch gradients is the gradient of the row, so the trajectory is test_trajectory_against_torch's, under its allowances
    (losses max(FACTOR e32, 2^-21), tensors max(FACTOR e32, spacing); FACTOR = 4).  Measured on one MI355X: the largest tensor ratio 1.78 (fc1.bias), the largest loss error 0.22 of
    its allowance."""
    from gpd_amd import api
    C, G = 3, 2
    st0 = api.init_state(C, 1)
    img, lab = tr.images(C), tr.labels()
    l64, s64, el32, e32 = tr.trajectory_yardstick(st0, img, lab, ROWS)
    with _Rig(C, G) as rig:
        for t in rig.trainers:
            t.set_data(img, lab)
        rig.trainers[0].set_state(st0)
        rig.group.broadcast(0)
        losses, each = rig.group.steps(np.stack([ROWS[:, :4], ROWS[:, 4:]]))
        state = rig.trainers[1].get_state()
        assert rig.group.verify() == 0
    bad, worst = [], 0.0
    for s in range(len(ROWS)):
        err, allow = abs(float(losses[s]) - l64[s]), max(tr.FACTOR * el32[s], 2.0 ** -21)
        print("4 + 4 step %d: loss f64 %.9g  device %.9g  e32 = %.3g  error = %.3g  allowance = %.3g  fraction %.2f" % (s, l64[s], losses[s], el32[s], err, allow, err / allow))
        if err > allow:
            bad.append((s, err, allow))
    for k in api.TORCH_KEYS:
        err = float(np.abs(state[k].astype(np.float64) - s64[k]).max())
        allow = max(tr.FACTOR * e32[k], float(np.spacing(np.float32(np.abs(s64[k]).max()))))
        ratio = err / e32[k] if e32[k] else 0.0
        worst = max(worst, ratio)
        print("4 + 4 %-12s e32 = %.3g  device error = %.3g  ratio = %.2f  allowance = %.3g" % (k, e32[k], err, ratio, allow))
        if err > allow:
            bad.append((k, err, allow))
    print("4 + 4 largest ratio %.2f" % worst)
    assert not bad, bad


# ---- 4. across steps and calls ----------------------------------------------------------------------------------------------------

def test_steps_and_calls_give_the_same_bytes():
    """G = 3 (every replica both reads from and is read by two peers): one call of 6 steps, six calls of 1 step, and the first
    again.  A backward pass that overwrote a buffer a peer still read, or a gather row refilled too early, would differ."""
    C, G, b = 3, 3, 2
    idx = _indices(C, G, b, 6)
    with _Rig(C, G) as rig:
        _fill(rig, C, G)
        runs = []
        for calls in (1, 6, 1):
            _start(rig, C, "adam")
            per = 6 // calls
            got = [rig.group.steps(idx[:, i * per:(i + 1) * per]) for i in range(calls)]
            losses, each = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got], axis=1)
            assert rig.group.verify() == 0
            runs.append((losses.tobytes(), each.tobytes(), [_everything(t) for t in rig.trainers]))
    assert runs[0][2][0]["count"] == 6
    assert runs[0] == runs[1], "six calls of one step differ from one call of six"
    assert runs[0] == runs[2], "the same call again differs"
    assert len(set(np.frombuffer(runs[0][0], np.float32).tolist())) == 6


# ---- 5. broadcast and verify ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["adam", "caffe"])
def test_broadcast_and_verify(name):
    C, G, b = 1, 3, 2
    idx = _indices(C, G, b)
    with _Rig(C, G, **_kw(name)) as rig:
        _fill(rig, C, G)
        assert rig.group.verify() == 0  # fresh trainers: all zeros
        rig.trainers[0].set_state(_init(C, name))
        assert rig.group.verify() > 0
        rig.group.broadcast(0)
        assert rig.group.verify() == 0
        n = 500 * C + 3626572
        assert rig.group.last_bytes()[0] == (G - 1) * 4 * n * (2 if name == "caffe" else 3)  # verify: replica 0's buffers to every other
        rig.trainers[0].steps(idx[0, :2])  # alone, twice: legal
        differ = rig.group.verify()
        assert differ > 2 * 1000  # most words of three (two) buffers in two replicas, and the two counts
        rig.group.broadcast(0)
        want = _everything(rig.trainers[0])
        assert want["count"] == 2
        for t in rig.trainers[1:]:
            assert _everything(t) == want
        assert rig.group.verify() == 0
        rig.trainers[1].steps(idx[1, :1])
        assert rig.group.verify() > 0
        rig.group.broadcast(1)  # any replica can be the source
        assert rig.group.verify() == 0 and _everything(rig.trainers[0])["count"] == 3


def test_verify_counts_words():
    """One word changed in one tensor of one replica is one; a count alone is one."""
    C, G = 1, 2
    from gpd_amd import api
    with _Rig(C, G) as rig:
        st = {k: np.array(v) for k, v in api.init_state(C, 1).items()}
        rig.trainers[0].set_state(st)
        rig.group.broadcast(0)
        st["fc2.bias"][1] = np.nextafter(st["fc2.bias"][1], np.float32(9))  # the buffer's last float
        st["conv1.weight"].reshape(-1)[0] += 1
        rig.trainers[1].set_state(st)
        assert rig.group.verify() == 2
        rig.trainers[1].set_solver_state(dict(rig.trainers[1].get_solver_state(), count=7))
        assert rig.group.verify() == 3


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_everything_usable():
    from gpd_amd import api
    case = CASES[0]
    C, G, b, name = case
    idx = _indices(C, G, b)
    with _Rig(C, G, max_batch=[8, 4]) as rig, _Rig(1, 1, group=False) as other_c, _Rig(C, 1, group=False, recipe=_recipe("caffe")) as other_r:
        _fill(rig, C, G)

        def still_works():
            _start(rig, C, name)
            losses, each = rig.group.steps(idx)
            _assert_is_composed(rig, losses, each, case)

        still_works()
        t0, t1 = rig.trainers
        with pytest.raises(api.GpdHipError, match="trainer 1 has 1 channels, trainer 0 has 3"):
            api.TrainerGroup([t0, other_c.trainers[0]])
        still_works()
        with pytest.raises(api.GpdHipError, match="trainer 1 is trainer 0 again"):
            api.TrainerGroup([t0, t0])
        still_works()
        same_ctx = api.Trainer(rig.ctxs[0], max_batch=4)
        try:
            with pytest.raises(api.GpdHipError, match="trainers 0 and 1 share a context"):
                api.TrainerGroup([t0, same_ctx])
        finally:
            same_ctx.close()
        still_works()
        with pytest.raises(api.GpdHipError, match="recipe of trainer 1 differs"):
            api.TrainerGroup([t0, other_r.trainers[0]])
        still_works()
        other_lr = api.Trainer(other_r.ctxs[0], max_batch=4, lr=2e-3)
        try:
            with pytest.raises(api.GpdHipError, match="gpd_train_params of trainer 1 differ"):
                api.TrainerGroup([t0, other_lr])
        finally:
            other_lr.close()
        with pytest.raises(api.GpdHipError, match="a null argument, or 0 trainers"):
            api.TrainerGroup([])
        still_works()
        before = [_everything(t) for t in rig.trainers]
        with pytest.raises(api.GpdHipError, match="batch 5 is outside 1 .. max_batch = 4 of replica 1"):
            rig.group.steps(np.zeros((G, 1, 5), np.int32))
        n1 = len(tr.labels()[1::G])
        outside = np.array(idx)
        outside[1, 1, 2] = n1
        with pytest.raises(api.GpdHipError, match="replica 1: index %d at position %d is outside the resident set of %d images" % (n1, b + 2, n1)):
            rig.group.steps(outside)
        assert [_everything(t) for t in rig.trainers] == before and rig.group.verify() == 0  # nothing was launched
        still_works()


# ---- 7. no parameter crosses to the host ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,G,b,steps", [(3, 3, 2, 2), (15, 2, 2, 3)])
def test_bytes_moved(C, G, b, steps):
    from gpd_amd import api
    with _Rig(C, G) as rig:
        _fill(rig, C, G)
        _start(rig, C, "adam")
        rig.group.steps(_indices(C, G, b)[:, :steps])
        between, host = rig.group.last_bytes()
    assert host <= 4 * G * steps * b + 4 * G * steps + 4096, host
    n = 500 * C + 3626572
    first = api.train_group_slices(n, G)
    ops = api.train_group_schedule(G, steps)
    copies = ops[ops["kind"] == api.OP_COPY]
    implied = int(sum(4 * (first[s + 1] - first[s]) for s in copies["slice"]))
    assert between == implied == steps * 2 * (G - 1) * 4 * n, (between, implied)


# ---- 8. the tool ------------------------------------------------------------------------------------------------------------------

def _read_dir(d):
    from gpd_amd import torch_export
    return {name: (d / name).read_bytes() for name in sorted(torch_export.FILES.values()) + ["network.cfg"]}


def test_the_tool(tmp_path, capsys):
    from gpd_amd import api, torch_export, train
    C, n, batch, seed = 1, 32, 8, 0
    img, lab = tr.images(C)[:n], tr.labels()[:n]
    data = tmp_path / "data"
    data.mkdir()
    np.save(data / "train_images.npy", img)
    np.save(data / "train_labels.npy", lab)
    assert train.main([str(data), "--devices", "0,0", "--batch", str(batch), "--epochs", "1", "--out", str(tmp_path / "group")]) == 0
    assert "over 2 replicas" in capsys.readouterr().out
    # the same shards, orders and steps through TrainerGroup
    G, b = 2, batch // 2
    with _Rig(C, G, max_batch=b) as rig:
        for r, t in enumerate(rig.trainers):
            t.set_data(img[r::G], lab[r::G])
        rig.trainers[0].set_state(api.init_state(C, seed))
        rig.group.broadcast(0)
        orders = [api.shuffle_orders((seed + 1000003 * (r + 1)) & 0xFFFFFFFF, [n // G])[0] for r in range(G)]
        assert orders[0].tolist() != orders[1].tolist()
        per = (n // G) // b
        rig.group.steps(np.stack([o[:per * b].reshape(per, b) for o in orders]))
        torch_export.export(rig.trainers[1].get_state(), str(tmp_path / "want_group"))
    assert _read_dir(tmp_path / "group") == _read_dir(tmp_path / "want_group")
    # without --devices: the single-device route as it was — one order over the whole set, the short last batch kept
    n1 = 28
    np.save(data / "train_images.npy", img[:n1])
    np.save(data / "train_labels.npy", lab[:n1])
    assert train.main([str(data), "--batch", str(batch), "--epochs", "1", "--out", str(tmp_path / "single")]) == 0
    with _Rig(C, 1, group=False, max_batch=batch) as rig:
        t = rig.trainers[0]
        t.set_state(api.init_state(C, seed))
        t.set_data(img[:n1], lab[:n1])
        order = api.shuffle_orders(seed, [n1])[0]
        t.steps(order[:24].reshape(3, 8))
        t.steps(order[24:].reshape(1, 4))
        torch_export.export(t.get_state(), str(tmp_path / "want_single"))
    assert _read_dir(tmp_path / "single") == _read_dir(tmp_path / "want_single")
    for argv, text in ((["--generate", "x.cfg", "--devices", "0,0"], "--generate with --devices"), ([str(data), "--devices", "0,0,0"], "divisible")):
        with pytest.raises(SystemExit):
            train.main(argv + ["--batch", "8", "--out", str(tmp_path / "no")])
        assert text in capsys.readouterr().err
