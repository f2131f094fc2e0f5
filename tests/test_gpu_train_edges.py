"""gpd_hip_train_* where test_gpu_train.py does not reach: the saturated branch of head_kernel one image at a
time against a float64 formula and a derived relative bound; gradients on batches that span both head branches, at other input
scales, with a repeated index and at 257 images; every step of a trajectory and its final state against torch.optim.Adam; Adam
over 40 steps at other settings; eval in a short last chunk, on the second set and on ties; step_timed; the refusals of create.

Truth: torch in float64 on the CPU (train_ref.py), for the head a float64 formula on the device's own float32 logits.  Yardstick:
train_ref's two float32 runs, factor 4.  Each test fixes its condition on the reference first.  Measured figures: profiles/NOTES.md §L.
"""
import functools
import time

import numpy as np
import pytest

import lenet_torch_ref as ltr
import train_ref as tr

pytestmark = pytest.mark.gpu


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


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


# ---- A. the head, one image at a time ----------------------------------------------------------------------------------------

_ONE = np.float32(1.0)
# |d|: near 0, the middle of the tanh branch, around the branch cut at 1 (the two neighbours of 1.0, 1.0 itself, and 2 ulps / 4 ulps
# of 1 further out, which stay on their side of 1 whatever the last bit of the logits does), the saturated branch, 16.6 / 17.4
# (where 1 + e stops moving), 87.2 .. 103.5 (e^-|d| becomes a float32 denormal, then 0), 110
HEAD_TARGETS = (1e-4, 0.5, 1.0 - 2.0 ** -22, float(np.nextafter(_ONE, np.float32(0))), 1.0, float(np.nextafter(_ONE, np.float32(2))),
                1.0 + 2.0 ** -21, 2.0, 8.0, 16.6, 17.4, 40.0, 87.2, 87.5, 95.0, 103.2, 103.5, 110.0)
HEAD_REL = 16 * 2.0 ** -24   # expf, log1pf or tanhf, one add and one divide at a few ulps each
HEAD_ABS = 2 * 2.0 ** -149   # two denormal spacings
F32_MIN_NORMAL = 2.0 ** -126


def _head_ok(dev, want, d32):
    """-> (passes, fraction of the bound used): |dev - want| <= want * (spacing(|d|) / 2 + 16 * 2^-24) + 2 * 2^-149 — the first
    term is the one rounding of z1 - z0 the kernel is entitled to; below the smallest normal float32, exactly 0 passes too"""
    if not np.isfinite(dev) or dev < 0:
        return False, float("inf")
    allow = want * (float(np.spacing(np.float32(abs(d32)))) / 2 + HEAD_REL) + HEAD_ABS
    err = abs(float(dev) - want)
    if want < F32_MIN_NORMAL and dev == 0:
        return True, 0.0
    return err <= allow, err / allow


@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_head_probes(offset):
    """B = 1: the fc2.bias gradient IS dlogits = (+-p_false, -+p_false) and the loss is loss_b.  One image resident twice, once
    under each label; fc2.bias = (o, o + target - d0) puts the device's d = z1 - z0 on the target, with both signs."""
    C = 1
    img = np.repeat(tr.images(C)[:1], 2, axis=0)
    lab = np.array([0, 1], np.uint8)
    st = {k: np.array(v) for k, v in ltr.state(C).items()}
    t0 = time.time()
    worst, bad, band, near_one = {"loss": 0.0, "grad": 0.0}, [], [], []
    with _Rig(C, max_batch=4) as t:
        t.set_data(img, lab)
        st["fc2.bias"] = np.zeros(2, np.float32)
        t.set_state(st)
        z = t.eval(np.array([0], np.int32))[0][0]
        d0 = float(z[1]) - float(z[0])
        for target in HEAD_TARGETS:
            for sign in (1.0, -1.0):
                T = sign * target
                b1 = offset + T - d0
                # around the cut the last bit of the logits decides the branch: step fc2.bias[1] by what is missing (twice at most)
                for attempt in range(3 if (offset == 0 and abs(target - 1) < 1e-6) else 1):
                    st["fc2.bias"] = np.array([offset, b1], np.float32)
                    t.set_state(st)
                    z = t.eval(np.array([0], np.int32))[0][0]
                    d32 = np.float32(z[1]) - np.float32(z[0])  # the kernel's d: one float32 subtraction
                    if float(d32) == float(np.float32(T)):
                        break
                    b1 += T - float(d32)
                # the condition, on the logits the device returned: d is on the target to the rounding of the two 500-term chains
                # (with the offset each term rounds at the spacing of 1000: a random walk of a few spacings)
                ulp = float(np.spacing(np.float32(max(abs(float(z[0])), abs(float(z[1])), abs(T)))))
                assert abs(float(d32) - T) <= 64 * ulp, (offset, T, z)
                if abs(target - 1) < 1e-6:
                    near_one.append(abs(float(d32)))
                d64, loss64, p64 = tr.head64(np.stack([z, z]), lab)
                for i in (0, 1):
                    g, loss = t.gradients(np.array([i], np.int32))
                    gb = g["fc2.bias"]
                    ok_l, f_l = _head_ok(loss, float(loss64[i]), d32)
                    ok_g, f_g = _head_ok(abs(float(gb[1])), float(p64[i]), d32)
                    # antisymmetric by construction, the true class pulled up
                    ok_s = gb[0] == -gb[1] and abs(float(gb[0])) == abs(float(gb[1])) and (gb[1] <= 0 if lab[i] else gb[1] >= 0)
                    if not (ok_l and ok_g and ok_s):
                        bad.append((offset, T, int(lab[i]), float(d32), loss, float(loss64[i]), gb.tolist(), float(p64[i])))
                    worst["loss"], worst["grad"] = max(worst["loss"], f_l), max(worst["grad"], f_g)
                    if 0 < min(loss64[i], p64[i]) < F32_MIN_NORMAL:
                        band.append((T, int(lab[i]), loss, float(loss64[i]), abs(float(gb[1])), float(p64[i])))
                    # the same image four times: / 4 and the four adds give p_false back exactly while p_false / 4 is a normal
                    # float32 (g + g and 4 g are exact, and 3 g rounds by less than half a spacing of 4 g, or ties to 4 g)
                    if min(p64[i], loss64[i]) >= 2.0 ** -120:
                        g4, loss4 = t.gradients(np.array([i] * 4, np.int32))
                        if g4["fc2.bias"].tobytes() != gb.tobytes() or loss4 != loss:
                            bad.append(("four times", offset, T, int(lab[i]), g4["fc2.bias"].tolist(), gb.tolist(), loss4, loss))
    for row in band:
        print("offset %g underflow band: d = %g, label %d: loss %.9g (f64 %.9g), |grad| %.9g (f64 %.9g)" % ((offset,) + row))
    print("offset %g: %d probes, largest fraction of the bound: loss %.3f, gradient %.3f; %.1f s"
          % (offset, 4 * len(HEAD_TARGETS), worst["loss"], worst["grad"], time.time() - t0))
    assert not bad, bad
    if offset == 0:  # both sides of the cut were visited, each within 2^-20 of it
        assert min(near_one) < 1 <= max(near_one) and max(abs(v - 1) for v in near_one) <= 2.0 ** -20, near_one


# ---- B. gradients through the yardstick ---------------------------------------------------------------------------------------

def _check(what, C, img, lab, idx, st, max_batch=64, **kw):
    """tr.check_gradients of set (img, lab) gathered by idx under state st -> (gradients, loss)"""
    scale = kw.get("input_scale", 1.0 / 256)
    g64, l64, e32, el32 = tr.yardstick(st, img[idx], lab[idx], scale)
    with _Rig(C, max_batch=max_batch, **kw) as t:
        t.set_state(st)
        t.set_data(img, lab)
        got, loss = t.gradients(idx)
    worst = tr.check_gradients(what, got, loss, g64, l64, e32, el32)
    print("%s largest ratio %.2f" % (what, worst))
    return got, loss


def _scaled_head(C, B, a, centre):
    """ltr.state(C) with fc2 scaled by a and fc2.bias[1] moved so that d = a * (d0 - centre) -> (state, float64 margins d)"""
    st = {k: np.array(v) for k, v in ltr.state(C).items()}
    st["fc2.weight"] = (st["fc2.weight"].astype(np.float64) * a).astype(np.float32)
    b = st["fc2.bias"].astype(np.float64) * a
    b[1] -= a * centre
    st["fc2.bias"] = b.astype(np.float32)
    z = tr.logits64(st, tr.images(C)[:B])
    return st, z[:, 1] - z[:, 0]


def _margins0(C, B):
    z = tr.logits64(ltr.state(C), tr.images(C)[:B])
    return z[:, 1] - z[:, 0]


def test_both_head_branches_in_one_batch():
    C, B = 3, 16
    img, lab = tr.images(C)[:B], tr.labels()[:B]
    d0 = _margins0(C, B)
    centre = float(np.median(d0))
    # the scale (78) puts the third largest |d0 - median| on 1.5: the largest alone would leave one image beyond the cut.
    # The margins of the fixture lie within +-0.044 of their median, so every d is 78 times a small difference, and so is the
    # float32 error of the forward pass in it — torch's as well: the loss of this batch is the one figure of this file that sits
    # at its allowance (device 4.7e-7 against the floor of 2^-21 = 4.8e-7, torch's two float32 runs 1.1e-7 and 2.3e-7; NOTES §L)
    st, d = _scaled_head(C, B, 1.5 / float(np.sort(np.abs(d0 - centre))[-3]), centre)
    print("margins:", np.array2string(np.sort(d), precision=3), "labels", lab.tolist())
    inner, outer = np.abs(d) < 0.9, np.abs(d) > 1.1
    assert inner.sum() >= 2 and outer.sum() >= 2 and (d > 0).any() and (d < 0).any()
    for side in (inner, outer):
        assert set(lab[side].tolist()) == {0, 1}
    _check("C = 3, B = 16, both branches:", C, img, lab, np.arange(B, dtype=np.int32), st)


def test_saturated_batch():
    """Every |d| > 50, both signs: the centre is the middle of the widest gap of the sorted margins that leaves a wrong-class
    image of each label (label 1 with d < 0, label 0 with d > 0)."""
    C, B = 3, 16
    img, lab = tr.images(C)[:B], tr.labels()[:B]
    d0 = _margins0(C, B)
    s = np.sort(d0)
    best = None
    for lo, hi in zip(s[:-1], s[1:]):
        c = 0.5 * (lo + hi)
        if ((lab == 1) & (d0 < c)).any() and ((lab == 0) & (d0 > c)).any() and (best is None or hi - lo > best[1]):
            best = (c, hi - lo)
    assert best is not None
    st, d = _scaled_head(C, B, 110.0 / best[1], best[0])
    print("margins:", np.array2string(np.sort(d), precision=1), "labels", lab.tolist())
    assert (np.abs(d) > 50).all() and ((lab == 1) & (d < 0)).any() and ((lab == 0) & (d > 0)).any()
    _check("C = 3, B = 16, every |d| > 50:", C, img, lab, np.arange(B, dtype=np.int32), st)


@pytest.mark.parametrize("scale", [1.0 / 255, 1.0])
def test_input_scale(scale):
    import torch
    from gpd_amd import api
    C, B = 3, 5
    img, lab, st = tr.images(C), tr.labels(), ltr.state(C)
    idx = np.array([69, 3, 41, 17, 8], np.int32)
    g64, l64, e32, el32 = tr.yardstick(st, img[idx], lab[idx], scale)
    # what install() then scores with: the float32 forward error (in order on several threads, reversed on one) on logit1 - logit0
    truth = tr.logits64(st, img, scale)
    t64 = truth[:, 1] - truth[:, 0]
    a = ltr.forward(st, img, torch.float32, input_scale=scale)["score"]
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        b = ltr.forward(st, img[::-1], torch.float32, input_scale=scale)["score"][::-1]
    finally:
        torch.set_num_threads(before)
    f32 = max(float(np.abs(a - t64).max()), float(np.abs(b - t64).max()))
    with _Rig(C, input_scale=scale) as t:
        t.set_state(st)
        t.set_data(img, lab)
        got, loss = t.gradients(idx)
        logits, _ = t.eval(n=len(img))
        ctx = t._ctx
        t.install()
        ctx.set_lenet_mode(api.LENET_F32_CHAIN)
        score = ctx.score(img)
    worst = tr.check_gradients("input_scale %.6g:" % scale, got, loss, g64, l64, e32, el32)
    dev = logits[:, 1].astype(np.float64) - logits[:, 0]
    err, err64 = float(np.abs(score.astype(np.float64) - dev).max()), float(np.abs(dev - t64).max())
    print("input_scale %.6g: largest ratio %.2f; |chain score - (logit1 - logit0)| = %.3g, |eval - f64| = %.3g, float32 forward error %.3g"
          % (scale, worst, err, err64, f32))
    assert err <= 4 * f32 and err64 <= 4 * f32


def test_repeated_index():
    C = 12
    _check("C = 12, indices 4 9 4 4 0:", C, tr.images(C), tr.labels(), np.array([4, 9, 4, 4, 0], np.int32), ltr.state(C))


def test_batch_of_257():
    """The smallest batch at which block_sum loops over the losses and head_kernel starts a fifth block."""
    C, B = 1, 257
    idx = np.arange(B, dtype=np.int32)[::-1].copy()
    _check("C = 1, B = 257:", C, tr.images(C, n=B), tr.labels(B), idx, ltr.state(C), max_batch=B)


def test_create_refuses_and_the_context_lives():
    from gpd_amd import api
    C = 1
    img, lab, st = tr.images(C), tr.labels(), ltr.state(C)
    idx = np.array([5, 2], np.int32)
    ctx = api.Context(api.default_params(C))
    try:
        def gradients(**kw):
            t = api.Trainer(ctx, **kw)
            try:
                t.set_state(st)
                t.set_data(img[:8], lab[:8])
                return t.gradients(idx)
            finally:
                t.close()

        want, want_loss = gradients()
        with pytest.raises(api.GpdHipError, match="max_batch 1025 is outside 1 .. 1024"):
            api.Trainer(ctx, max_batch=1025)
        for bad in (dict(lr=-1.0), dict(beta1=1.0), dict(beta2=-0.1), dict(eps=float("nan")), dict(weight_decay=float("inf")), dict(input_scale=0.0)):
            with pytest.raises(api.GpdHipError, match="out of range"):
                api.Trainer(ctx, **bad)
            got, loss = gradients()
            assert loss == want_loss and _same(got, want), bad
        got, loss = gradients(max_batch=1024)  # the largest accepted: every buffer is sized by it, the arithmetic is not
        assert loss == want_loss and _same(got, want)
    finally:
        ctx.close()


def test_sets_come_and_go():
    from gpd_amd import api
    C = 3
    img, lab, st = tr.images(C), tr.labels(), ltr.state(C)
    idx = np.array([1, 66, 7, 30, 69], np.int32)
    with _Rig(C) as t:
        t.set_state(st)
        t.set_data(img, lab)
        want, want_loss = t.gradients(idx)
    with _Rig(C) as t:
        t.set_state(st)
        t.set_data(img[:8], lab[:8])
        t.gradients(idx[[0, 2]])
        t.set_data(img[:0], lab[:0])
        with pytest.raises(api.GpdHipError, match="no training set"):
            t.gradients(idx[[0, 2]])
        t.set_data(img[:8], lab[:8])
        with pytest.raises(api.GpdHipError, match="index 66 at position 1"):
            t.gradients(idx)
        t.set_data(img, lab)  # replaced by a larger one
        got, loss = t.gradients(idx)
    assert loss == want_loss and _same(got, want)


# ---- C. a trajectory against torch ---------------------------------------------------------------------------------------------

ROWS = np.arange(48, dtype=np.int32).reshape(6, 8)
OTHER = dict(lr=3e-3, beta1=0.5, beta2=0.9, eps=1e-3, weight_decay=0.0, input_scale=1.0 / 255)


@functools.lru_cache(maxsize=None)
def _device_steps(C, other):
    from gpd_amd import api
    with _Rig(C, **(OTHER if other else {})) as t:
        t.set_state(api.init_state(C, 1))
        t.set_data(tr.images(C), tr.labels())
        losses = t.steps(ROWS)
        return losses, t.get_state()


@pytest.mark.parametrize("C,other", [(3, False), (15, False), (3, True)])
def test_trajectory_against_torch(C, other):
    from gpd_amd import api
    st0 = api.init_state(C, 1)
    lab = tr.labels()
    assert len({tuple(lab[r].tolist()) for r in ROWS}) == len(ROWS)  # the labels differ from row to row: a wrong row shows
    l64, s64, el32, e32 = tr.trajectory_yardstick(st0, tr.images(C), lab, ROWS, OTHER if other else None)
    losses, state = _device_steps(C, other)
    assert losses.shape == (len(ROWS),) and losses.dtype == np.float32
    bad = []
    for s in range(len(ROWS)):
        err, allow = abs(float(losses[s]) - l64[s]), max(tr.FACTOR * el32[s], 2.0 ** -21)
        print("C = %d%s step %d: loss f64 %.9g  device %.9g  e32 = %.3g  error = %.3g  allowance = %.3g" % (C, " other" if other else "", s, l64[s], losses[s], el32[s], err, allow))
        if err > allow:
            bad.append((s, err, allow))
    for k in api.TORCH_KEYS:
        err = float(np.abs(state[k].astype(np.float64) - s64[k]).max())
        allow = max(tr.FACTOR * e32[k], float(np.spacing(np.float32(np.abs(s64[k]).max()))))
        moved = float(np.abs(s64[k] - st0[k]).max())
        print("C = %d%s %-12s e32 = %.3g  device error = %.3g  ratio = %.2f  allowance = %.3g  moved by %.3g" % (C, " other" if other else "", k, e32[k], err, err / e32[k] if e32[k] else 0.0, allow, moved))
        if err > allow:
            bad.append((k, err, allow))
        assert moved > 1e-3, (k, moved)
    assert not bad, bad


def test_three_ways_to_step():
    """One steps() call, six gradients() + apply() pairs and six step_timed() calls: the same bytes.  (step_timed returns no
    loss; its loss is the one its state was made from.)"""
    from gpd_amd import api
    C = 3
    losses, state = _device_steps(C, False)
    names = [api.lib().gpd_hip_train_kernel_name(i).decode() for i in range(18)]
    assert all(names) and len(set(names)) == 18 and api.lib().gpd_hip_train_kernel_name(18) == b""
    with _Rig(C) as t:
        t.set_data(tr.images(C), tr.labels())
        t.set_state(api.init_state(C, 1))
        pair_losses = []
        for row in ROWS:
            g, loss = t.gradients(row)
            t.apply(g)
            pair_losses.append(loss)
        pairs = t.get_state()
        t.set_state(api.init_state(C, 1))
        for row in ROWS:
            times = t.step_timed(row)
            assert [n for n, _ in times] == names
            assert all(np.isfinite(ms) and ms >= 0 for _, ms in times), times
        timed = t.get_state()
    assert np.array(pair_losses, np.float32).tobytes() == losses.tobytes()
    for k in state:
        assert state[k].tobytes() == pairs[k].tobytes(), k
        assert state[k].tobytes() == timed[k].tobytes(), k


# ---- D. Adam over more steps and other settings -------------------------------------------------------------------------------

ADAM_STEPS, ADAM_SETS = 40, 8


@functools.lru_cache(maxsize=None)
def _adam_inputs():
    """test_adam_against_torch's generator at C = 1: ADAM_SETS gradient sets (the draws are the cost, and 40 fresh sets say no
    more about 40 bias corrections than these do) -> (the initial state, the sets)"""
    from gpd_amd import api
    st = api.init_state(1, 3)
    rng = np.random.RandomState(5)
    sets = []
    for _ in range(ADAM_SETS):
        g = {}
        for k in api.TORCH_KEYS:
            a = (rng.randn(*st[k].shape) * 10.0 ** rng.uniform(-6, -1, st[k].shape)).astype(np.float32)
            r = rng.rand(*st[k].shape)
            a[r < 0.2] = 0.0           # exact zeros: only the weight decay moves these
            a[(r >= 0.2) & (r < 0.3)] = 1e-12
            a[(r >= 0.3) & (r < 0.35)] = -1e-12
            g[k] = a
        sets.append(g)
    return st, sets


def _adam_grads(steps=ADAM_STEPS):
    """step s takes set s mod ADAM_SETS with the sign (-1)^(s div ADAM_SETS)"""
    sets = _adam_inputs()[1]
    for s in range(steps):
        g = sets[s % ADAM_SETS]
        yield {k: -v for k, v in g.items()} if (s // ADAM_SETS) % 2 else g


def _torch_adam(st, dtype, hyper):
    import torch
    h = dict(tr.HYPER, **hyper)
    ps = [torch.from_numpy(np.array(st[k])).to(dtype).requires_grad_(True) for k in st]
    opt = torch.optim.Adam(ps, lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=h["weight_decay"])
    for g in _adam_grads():
        for p, k in zip(ps, st):
            p.grad = torch.from_numpy(np.array(g[k])).to(dtype)
        opt.step()
    return {k: p.detach().numpy() for k, p in zip(st, ps)}


@pytest.mark.parametrize("hyper", [{}, dict(lr=1e-2, beta1=0.5, beta2=0.9, eps=1e-3, weight_decay=0.0), dict(beta1=0.0, beta2=0.0)],
                         ids=["defaults", "other", "betas0"])
def test_adam_forty_steps(hyper):
    import torch
    from gpd_amd import api
    st = _adam_inputs()[0]
    with _Rig(1, **hyper) as t:
        t.set_state(st)
        for s, g in enumerate(_adam_grads()):
            t.apply(g)
            if s == 2:
                three = t.get_state()
        got = t.get_state()
        t.set_state(st)  # the moments and the step count start again
        for g in _adam_grads(3):
            t.apply(g)
        again = t.get_state()
    assert _same(three, again)
    p64, p32 = _torch_adam(st, torch.float64, hyper), _torch_adam(st, torch.float32, hyper)
    bad = []
    for k in api.TORCH_KEYS:
        yard = float(np.abs(p32[k].astype(np.float64) - p64[k]).max())
        err = float(np.abs(got[k].astype(np.float64) - p64[k]).max())
        allow = max(4 * yard, float(np.spacing(np.float32(np.abs(st[k]).max()))))
        moved = float(np.abs(p64[k] - st[k]).max())
        print("Adam %s %-12s torch f32 error %.3g  device error %.3g  ratio %.2f  allowance %.3g  moved by %.3g" % (hyper, k, yard, err, err / yard if yard else 0.0, allow, moved))
        if err > allow:
            bad.append((k, err, allow))
        assert moved > 1e-3
    assert not bad, bad


def test_adam_lr_zero_moves_nothing():
    st = _adam_inputs()[0]
    with _Rig(1, lr=0.0) as t:
        t.set_state(st)
        for g in _adam_grads():
            t.apply(g)
        assert _same(t.get_state(), st)


# ---- E. eval --------------------------------------------------------------------------------------------------------------------

def test_eval_chunks_sets_and_ties():
    import torch
    C, n = 3, 70
    img, lab, st = tr.images(C), tr.labels(), ltr.state(C)
    rev = np.arange(n)[::-1]
    perm = np.random.RandomState(21).randint(0, n, n).astype(np.int32)  # with repeats
    perm[[0, 63, 64, 69]] = [69, 5, 5, 0]  # image 5 on both sides of the chunk boundary
    assert len(set(perm.tolist())) < n
    truth = tr.logits64(st, img)
    # the float32 forward error on either logit: in order on several threads, reversed on one
    f32a = tr.logits(st, img, torch.float32).astype(np.float64)
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        f32b = tr.logits(st, img[::-1], torch.float32).astype(np.float64)[::-1]
    finally:
        torch.set_num_threads(before)
    e32 = max(float(np.abs(f32a - truth).max()), float(np.abs(f32b - truth).max()))
    with _Rig(C, max_batch=64) as t:
        t.set_state(st)
        t.set_data(img, lab)
        t.set_data(img[::-1], lab[::-1], which=1)
        first = {w: t.eval(n=n, which=w) for w in (0, 1)}          # chunks of 64 + 6
        listed = {w: t.eval(perm, which=w) for w in (0, 1)}
        alone = [t.eval(np.array([i], np.int32))[0][0] for i in (0, 5, 63, 64, 69)]
        tie = {k: np.array(v) for k, v in st.items()}
        tie["fc2.weight"][:] = 0
        tie["fc2.bias"][:] = 0.25
        t.set_state(tie)
        tied = {w: t.eval(n=n, which=w) for w in (0, 1)}
    worst = 0.0
    for w, order in ((0, np.arange(n)), (1, rev)):
        for what, (logits, correct), ids in (("first 70", first[w], order), ("listed", listed[w], order[perm])):
            assert logits.shape == (n, 2) and logits.dtype == np.float32
            err = float(np.abs(logits - truth[ids]).max())
            worst = max(worst, err / e32)
            print("eval set %d %s: |logits - f64| = %.3g, float32 forward error %.3g, ratio %.2f, %d correct" % (w, what, err, e32, err / e32, correct))
            assert err <= 4 * e32
            assert correct == int(((logits[:, 1] > logits[:, 0]) == (lab[ids] == 1)).sum())
            # an image's logits are the same bytes wherever it stands
            assert logits.tobytes() == first[0][0][ids].tobytes(), (w, what)
        logits, correct = tied[w]
        assert (logits == 0.25).all() and correct == int((lab == 0).sum())  # a tie predicts class 0, as torch.max
    for i, z in zip((0, 5, 63, 64, 69), alone):
        assert z.tobytes() == first[0][0][i].tobytes(), i
    assert 0 < int((lab == 0).sum()) < n

