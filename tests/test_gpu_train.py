"""gpd_hip_train_* on the device: the gradients against torch autograd in float64 with torch's own float32 error
as the yardstick (train_ref.py), the pooling tie rule, Adam against torch.optim.Adam, that it learns, that it is reproducible
to the bit, that the trained network is the one the context then scores with, the refusals, and the command-line tool.

Measured on an MI355X (ratio = device error / e32, e32 = the larger error of two float32 torch runs against float64; the
allowance is 4): the figures are in profiles/NOTES.md.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import lenet_torch_ref as ltr
import train_ref as tr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Rig:
    """A context and a trainer on it, closed in order."""

    def __init__(self, C, **kw):
        from gpd_amd import api
        self.ctx = api.Context(api.default_params(C))
        try:
            self.trainer = api.Trainer(self.ctx, **kw)
        except Exception:
            self.ctx.close()
            raise

    def __enter__(self):
        return self.trainer

    def __exit__(self, *exc):
        self.trainer.close()
        self.ctx.close()


# ---- 1. gradients ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,B,max_batch", [(15, 64, 64), (1, 1, 64), (1, 5, 64), (3, 5, 64), (12, 5, 64), (15, 3, 64), (15, 70, 70)])
def test_gradients_against_float64_autograd(C, B, max_batch):
    img, lab, st = tr.images(C), tr.labels(), ltr.state(C)
    # the batch is gathered from the resident set: the last B images in an order that is not the stored one
    idx = (len(lab) - 1 - np.arange(B)).astype(np.int32)
    idx[: B // 2] = idx[: B // 2][::-1]
    g64, l64, e32, el32 = tr.yardstick(st, img[idx], lab[idx])
    with _Rig(C, max_batch=max_batch) as t:
        t.set_state(st)
        t.set_data(img, lab)
        got, loss = t.gradients(idx)
        again, loss2 = t.gradients(idx)
    worst = tr.check_gradients("C = %d, B = %d:" % (C, B), got, loss, g64, l64, e32, el32)
    print("C = %d, B = %d: largest ratio %.2f" % (C, B, worst))
    assert loss == loss2 and all(got[k].tobytes() == again[k].tobytes() for k in got)


# ---- 2. the tie rule ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,value", [(3, 0), (3, 200), (15, 0), (15, 37)])
def test_every_window_ties(C, value):
    """All-zero images and images of one constant byte: every pooling window of conv1 ties (and of conv2, where pool1 is
    constant per channel), so the whole gradient hangs on routing to the FIRST maximum in row-major order."""
    B = 5
    img = np.full((B, 60, 60, C), value, np.uint8)
    lab = np.array([0, 1, 1, 0, 1], np.uint8)
    st = ltr.state(C)
    g64, l64, e32, el32 = tr.yardstick(st, img, lab)
    with _Rig(C) as t:
        t.set_state(st)
        t.set_data(img, lab)
        got, loss = t.gradients(np.arange(B, dtype=np.int32))
    tr.check_gradients("C = %d, constant %d:" % (C, value), got, loss, g64, l64, e32, el32)
    if value == 0:
        assert not got["conv1.weight"].any()  # zero inputs: exactly zero
    assert np.abs(got["conv1.bias"]).max() > 0 and np.abs(got["conv2.weight"]).max() > 0  # the ties did carry gradient


# ---- 3. Adam -----------------------------------------------------------------------------------------------------------------

def _torch_adam(st, grads, dtype):
    import torch
    ps = [torch.from_numpy(np.array(st[k])).to(dtype).requires_grad_(True) for k in st]
    opt = torch.optim.Adam(ps, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4)
    for g in grads:
        for p, k in zip(ps, st):
            p.grad = torch.from_numpy(np.array(g[k])).to(dtype)
        opt.step()
    return {k: p.detach().numpy() for k, p in zip(st, ps)}


def test_adam_against_torch():
    import torch
    from gpd_amd import api
    C = 3
    st = api.init_state(C, 3)
    rng = np.random.RandomState(5)
    grads = []
    for step in range(3):
        g = {}
        for k in api.TORCH_KEYS:
            a = (rng.randn(*st[k].shape) * 10.0 ** rng.uniform(-6, -1, st[k].shape)).astype(np.float32)
            r = rng.rand(*st[k].shape)
            a[r < 0.2] = 0.0           # exact zeros: only the weight decay moves these
            a[(r >= 0.2) & (r < 0.3)] = 1e-12
            a[(r >= 0.3) & (r < 0.35)] = -1e-12
            g[k] = a
        grads.append(g)
    with _Rig(C) as t:
        t.set_state(st)
        for g in grads:
            t.apply(g)
        got = t.get_state()
        # set_state clears the moments and the step count: the same three steps again give the same bytes
        t.set_state(st)
        for g in grads:
            t.apply(g)
        again = t.get_state()
    p64, p32 = _torch_adam(st, grads, torch.float64), _torch_adam(st, grads, torch.float32)
    for k in api.TORCH_KEYS:
        yard = float(np.abs(p32[k].astype(np.float64) - p64[k]).max())
        err = float(np.abs(got[k].astype(np.float64) - p64[k]).max())
        allow = max(4 * yard, float(np.spacing(np.float32(np.abs(st[k]).max()))))
        print("Adam %-12s torch f32 error %.3g  device error %.3g  allowance %.3g  moved by %.3g" % (k, yard, err, allow, float(np.abs(p64[k] - st[k]).max())))
        assert err <= allow, (k, err, allow)
        assert np.abs(p64[k] - st[k]).max() > 1e-3  # three steps of about lr each
        assert got[k].tobytes() == again[k].tobytes()


# ---- 4 - 6. it learns, reproducibly, and the context scores with what was learnt ------------------------------------------------

def _run(C, calls):
    """The 40 steps of the learning task from init_state(C, 1) in a fresh trainer -> dict; calls: "one" (one call of 40 steps)
    or "forty" (40 calls of one step)"""
    from gpd_amd import api
    img, lab, idx = tr.learn_set(C)
    st0 = api.init_state(C, 1)
    with _Rig(C) as t:
        t.set_state(st0)
        t.set_data(img, lab)
        losses = t.steps(idx) if calls == "one" else np.concatenate([t.steps(row[None, :]) for row in idx])
        logits, correct = t.eval(n=256)
        out = dict(state0=st0, state=t.get_state(), losses=losses, logits=logits, correct=correct)
        if calls == "one":
            ctx = t._ctx
            t.install(ctx)
            ctx.set_lenet_mode(api.LENET_F32_CHAIN)
            out["score_chain"] = ctx.score(img)
            ctx.set_lenet_mode(api.LENET_SPLIT)
            out["score_split"] = ctx.score(img)
    return out


@functools.lru_cache(maxsize=None)
def _trained(C):
    return _run(C, "one")


@pytest.mark.parametrize("C", [3, 15])
def test_it_learns(C):
    import torch
    img, lab, idx = tr.learn_set(C)
    r = _trained(C)
    losses = r["losses"]
    acc = r["correct"] / 256.0
    print("C = %d: loss %.6g -> %.6g, training accuracy %.4f" % (C, losses[0], losses[-1], acc))
    assert losses.shape == (40,) and np.isfinite(losses).all()
    # the first loss is the initial state's: float64 forward of the first batch
    s = ltr.forward(r["state0"], img[idx[0]], torch.float64)["score"]
    want = float(np.log1p(np.exp(np.where(lab[idx[0]] == 1, -s, s))).mean())
    print("C = %d: first loss %.9g, float64 %.9g" % (C, losses[0], want))
    assert abs(float(losses[0]) - want) <= 2.0 ** -20
    assert acc >= 0.95
    assert r["correct"] == int(((r["logits"][:, 1] > r["logits"][:, 0]) == (lab == 1)).sum())
    if C == 3:
        assert losses[-1] < 0.1 * losses[0]
    else:
        assert losses[-1] < losses[0]


@pytest.mark.parametrize("C", [3, 15])
def test_reproducible_to_the_bit(C):
    a = _trained(C)
    b = _run(C, "one")
    c = _run(C, "forty")
    for other in (b, c):
        assert a["losses"].tobytes() == other["losses"].tobytes()
        assert a["logits"].tobytes() == other["logits"].tobytes()
        for k in a["state"]:
            assert a["state"][k].tobytes() == other["state"][k].tobytes(), k
    assert any(not np.array_equal(a["state"][k], a["state0"][k]) for k in a["state"])


@pytest.mark.parametrize("C", [3, 15])
def test_the_loop_closes(C):
    """Trainer.install: the context scores with the trained network.  The f32-chain mode and train_eval are two float32
    summation orders of the same network, so they may differ by what two float32 orders differ by: the yardstick is torch's
    float32 forward (in order on several threads, reversed on one) against float64, times 4, on logit1 - logit0."""
    import torch
    img, lab, _ = tr.learn_set(C)
    r = _trained(C)
    truth = tr.logits64(r["state"], img)
    t64 = truth[:, 1] - truth[:, 0]
    a = ltr.forward(r["state"], img, torch.float32)["score"]
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        b = ltr.forward(r["state"], img[::-1], torch.float32)["score"][::-1]
    finally:
        torch.set_num_threads(before)
    e32 = max(float(np.abs(a - t64).max()), float(np.abs(b - t64).max()))
    dev = r["logits"][:, 1] - r["logits"][:, 0]
    err = float(np.abs(r["score_chain"].astype(np.float64) - dev).max())
    print("C = %d: |chain score - (logit1 - logit0)| = %.3g, e32 = %.3g, ratio %.2f; |eval - f64| = %.3g, |split - f64| = %.3g"
          % (C, err, e32, err / e32, float(np.abs(dev - t64).max()), float(np.abs(r["score_split"] - t64).max())))
    assert err <= 4 * e32
    assert float(np.abs(dev - t64).max()) <= 4 * e32
    assert float(np.abs(r["score_split"] - t64).max()) <= 1e-4
    assert (((r["score_chain"] > 0) == (lab == 1)).mean()) >= 0.95


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_trainer_usable():
    from gpd_amd import api
    C = 3
    img, lab = tr.images(C)[:8], tr.labels()[:8]
    st = ltr.state(C)
    idx = np.arange(5, dtype=np.int32)
    with pytest.raises(api.GpdHipError, match="channels"):
        _Rig(C, channels=2)
    with pytest.raises(api.GpdHipError, match="max_batch"):
        _Rig(C, max_batch=0)
    with _Rig(C, max_batch=6) as t:
        t.set_state(st)
        t.set_data(img, lab)
        want, want_loss = t.gradients(idx)

        def still_fine():
            got, loss = t.gradients(idx)
            assert loss == want_loss and all(got[k].tobytes() == want[k].tobytes() for k in got)

        for bad in (np.nan, np.inf, -np.inf):
            broken = {k: v.copy() for k, v in st.items()}
            broken["fc1.weight"][123, 4567] = bad
            with pytest.raises(api.GpdHipError, match="fc1.weight.*non-finite"):
                t.set_state(broken)
            still_fine()  # the state was not touched
        two = lab.copy()
        two[3] = 2
        with pytest.raises(api.GpdHipError, match="label 2 of image 3"):
            t.set_data(img, two)
        still_fine()  # nor the data
        with pytest.raises(api.GpdHipError, match="index 8 at position 2"):
            t.gradients(np.array([0, 1, 8], np.int32))
        with pytest.raises(api.GpdHipError, match="index 8 at position 7"):
            t.steps(np.array([[0, 1, 2], [3, 4, 5], [6, 8, 7]], np.int32))
        with pytest.raises(api.GpdHipError, match="index -1"):
            t.eval(np.array([-1], np.int32))
        with pytest.raises(api.GpdHipError, match="batch 7 is outside 1 .. max_batch = 6"):
            t.gradients(np.arange(7, dtype=np.int32))
        with pytest.raises(api.GpdHipError, match="batch 7 is outside"):
            t.steps(np.arange(7, dtype=np.int32)[None, :])
        broken = {k: np.zeros_like(v) for k, v in st.items()}
        broken["conv1.bias"][0] = np.nan
        with pytest.raises(api.GpdHipError, match="non-finite"):
            t.apply(broken)
        with pytest.raises(api.GpdHipError, match="set 1 is empty"):
            t.eval(n=1, which=1)
        still_fine()
        assert t.get_state()["fc2.bias"].tobytes() == st["fc2.bias"].tobytes()  # no refused step moved anything
        # the second slot
        t.set_data(img[:3], lab[:3], which=1)
        logits, correct = t.eval(which=1, n=3)
        assert np.array_equal(logits, t.eval(np.arange(3, dtype=np.int32))[0]) and 0 <= correct <= 3


# ---- 8. the tool -------------------------------------------------------------------------------------------------------------

def test_the_tool_trains_and_exports(tmp_path):
    import torch
    from gpd_amd import api, torch_export
    C = 3
    img, lab, _ = tr.learn_set(C)
    data, out = tmp_path / "data", tmp_path / "net"
    data.mkdir()
    for prefix in ("train", "test"):
        np.save(str(data / (prefix + "_images.npy")), img)
        np.save(str(data / (prefix + "_labels.npy")), lab)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "gpd_amd.train", str(data), "--test", str(data), "--epochs", "10", "--seed", "1", "--out", str(out)],
                         capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=300)
    print(run.stdout[-3000:])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert run.stdout.count("accuracy:") == 10 and "[10,     4] loss:" in run.stdout
    # what it wrote is what torch_export writes from the model.pwf beside it: the same files, byte for byte
    again = tmp_path / "again"
    assert torch_export.main([str(out / "model.pwf"), str(again)]) == 0
    names = sorted(torch_export.FILES.values()) + ["network.cfg"]
    for name in names:
        assert (out / name).read_bytes() == (again / name).read_bytes(), name
    assert "layout = torch" in (out / "network.cfg").read_text()
    st = {k: np.fromfile(str(out / f), "<f4").reshape(s) for (k, f), s in zip(torch_export.FILES.items(), api.torch_state_shapes(C))}
    ctx = api.Context(api.default_params(C))
    try:
        ctx.set_lenet_torch(st)
        acc = float(((ctx.score(img) > 0) == (lab == 1)).mean())
    finally:
        ctx.close()
    print("the exported network scores the set with accuracy %.4f" % acc)
    assert acc >= 0.95
