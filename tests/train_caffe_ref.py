"""References of the Caffe recipe's tests (gpd_train_recipe), torch on the CPU, beside train_ref.py whose inputs,
yardstick and bound (images, labels, check_gradients, FACTOR) are used as they are.

  * the network of models/caffe/15channels/lenet_15_channels_train_val.prototxt: conv, 2 x 2 max-pool twice with NO ReLU
    behind the convolutions, channel-major flatten, fc1, ReLU, fc2 on image * input_scale, mean softmax cross-entropy;
  * Caffe's SGDSolver written out — d = g + (wd * decay_mult) * w, h = m * h + (lr * lr_mult) * d, w = w - h — NOT
    torch.optim.SGD, which folds the rate in after the momentum and so differs as soon as the rate changes;
  * the learning-rate policies in float64 with one rounding to float32;
  * xavier_bounds(): sqrt(3 / fan_in) per weight tensor.

float64 is the truth; float32 is the yardstick, taken twice — the batch in order on several threads, reversed on one.
"""
import functools

import numpy as np
import torch  # before the library is loaded (xavier_state loads it): the order every trainer test has had so far

from gpd_amd import api
from train_ref import FACTOR, check_gradients, images, labels  # noqa: F401  (re-exported: one yardstick)

SOLVER = dict(lr=0.01, momentum=0.9, weight_decay=5e-4, lr_policy="inv", gamma=1e-4, power=0.75, stepsize=1, input_scale=1.0 / 256)
POLICIES = dict(fixed=0, step=1, exp=2, inv=3)


def learning_rate64(policy, base_lr, it, gamma=1e-4, power=0.75, stepsize=1):
    """The rate of update `it` (0-based) in float64"""
    it = int(it)
    if policy == "fixed":
        return float(base_lr)
    if policy == "step":
        return float(base_lr) * float(gamma) ** float(it // int(stepsize))
    if policy == "exp":
        return float(base_lr) * float(gamma) ** float(it)
    if policy == "inv":
        return float(base_lr) * (1.0 + float(gamma) * float(it)) ** (-float(power))
    raise ValueError(policy)


def xavier_bounds(C):
    return {"conv1.weight": np.sqrt(3.0 / (25 * C)), "conv2.weight": np.sqrt(3.0 / 500), "fc1.weight": np.sqrt(3.0 / 7200), "fc2.weight": np.sqrt(3.0 / 500)}


@functools.lru_cache(maxsize=None)
def xavier_state(C, seed=1, bias=0.1):
    """init_xavier with the biases set to +-bias in turn (a zero bias leaves every all-zero window a four-way tie at 0)"""
    st = api.init_xavier(C, seed)
    for k in api.TORCH_KEYS:
        if k.endswith("bias"):
            st[k][:] = bias * (1 - 2 * (np.arange(st[k].size) % 2))
        st[k].setflags(write=False)
    return st


def _forward(t, img, dtype, input_scale):
    import torch
    import torch.nn.functional as F
    x = torch.from_numpy(np.array(np.transpose(np.asarray(img), (0, 3, 1, 2)), order="C")).to(dtype) * input_scale
    h = F.max_pool2d(F.conv2d(x, t["conv1.weight"], t["conv1.bias"]), 2)
    h = F.max_pool2d(F.conv2d(h, t["conv2.weight"], t["conv2.bias"]), 2)
    h = F.relu(F.linear(h.reshape(len(img), 7200), t["fc1.weight"], t["fc1.bias"]))
    return F.linear(h, t["fc2.weight"], t["fc2.bias"])


def _loss(t, img, lab, dtype, input_scale):
    import torch
    import torch.nn.functional as F
    return F.cross_entropy(_forward(t, img, dtype, input_scale), torch.from_numpy(np.asarray(lab).astype(np.int64)))


class _Threads:
    def __init__(self, n):
        self.n = n

    def __enter__(self):
        import torch
        self.before = torch.get_num_threads()
        if self.n:
            torch.set_num_threads(self.n)

    def __exit__(self, *exc):
        import torch
        torch.set_num_threads(self.before)


def autograd(state, img, lab, dtype, input_scale=1.0 / 256, reverse=False, threads=None):
    """-> ({key: gradient as numpy of dtype}, loss)"""
    import torch
    with _Threads(threads):
        order = np.arange(len(lab))[::-1].copy() if reverse else np.arange(len(lab))
        t = {k: torch.from_numpy(np.array(state[k])).to(dtype).requires_grad_(True) for k in api.TORCH_KEYS}
        loss = _loss(t, np.asarray(img)[order], np.asarray(lab)[order], dtype, input_scale)
        loss.backward()
        return {k: t[k].grad.numpy().copy() for k in api.TORCH_KEYS}, float(loss.item())


def yardstick(state, img, lab, input_scale=1.0 / 256):
    """train_ref.yardstick for this network -> (g64, loss64, {key: e32}, e32 of the loss)"""
    import torch
    g64, l64 = autograd(state, img, lab, torch.float64, input_scale)
    a, la = autograd(state, img, lab, torch.float32, input_scale)
    b, lb = autograd(state, img, lab, torch.float32, input_scale, reverse=True, threads=1)
    e32 = {k: max(float(np.abs(a[k].astype(np.float64) - g64[k]).max()), float(np.abs(b[k].astype(np.float64) - g64[k]).max())) for k in api.TORCH_KEYS}
    return g64, l64, e32, max(abs(la - l64), abs(lb - l64))


def logits(state, img, dtype, input_scale=1.0 / 256, reverse=False, threads=None):
    """The network's logits in `dtype` -> [n, 2] in the order of img"""
    import torch
    with _Threads(threads), torch.no_grad():
        t = {k: torch.from_numpy(np.array(state[k])).to(dtype) for k in api.TORCH_KEYS}
        x = np.asarray(img)[::-1] if reverse else np.asarray(img)
        z = _forward(t, x, dtype, input_scale).numpy()
        return z[::-1].copy() if reverse else z


def logits_yardstick(state, img, input_scale=1.0 / 256):
    """-> (logits64 [n, 2], e32 of either logit, e32 of z1 - z0): the float32 forward in order on several threads, reversed on one"""
    import torch
    z64 = logits(state, img, torch.float64, input_scale)
    runs = [logits(state, img, torch.float32, input_scale).astype(np.float64),
            logits(state, img, torch.float32, input_scale, reverse=True, threads=1).astype(np.float64)]
    d64 = z64[:, 1] - z64[:, 0]
    return z64, max(float(np.abs(z - z64).max()) for z in runs), max(float(np.abs((z[:, 1] - z[:, 0]) - d64).max()) for z in runs)


def caffe_sgd_trajectory(state, keys, loss_of, rows, dtype, hyper=None, lr_mult=None, decay_mult=None, reverse=False, threads=None):
    """Caffe's SGD rule over the tensors `keys` of `state`, one step per row of `rows`: loss_of(tensors, row, h) is the batch's
    loss under the tensors {key: torch tensor of dtype} and the solver settings h.  The update arithmetic is in `dtype` with the
    rate rounded to float32 first (what the solver hands to its update): d = g + (wd * decay_mult) w, hist = m * hist +
    (lr * lr_mult) * d, w = w - hist -> (every step's loss f64 [len(rows)], the final state {key: numpy})"""
    import torch
    h = dict(SOLVER, **(hyper or {}))
    lm = dict.fromkeys(keys, 1.0)
    lm.update(lr_mult or {})
    dm = dict.fromkeys(keys, 1.0)
    dm.update(decay_mult or {})
    f32 = dtype == torch.float32

    def num(x):  # a scalar of the run's precision
        return float(np.float32(x)) if f32 else float(x)

    with _Threads(threads):
        t = {k: torch.from_numpy(np.array(state[k])).to(dtype).requires_grad_(True) for k in keys}
        hist = {k: torch.zeros_like(t[k]) for k in keys}
        losses = []
        for it, row in enumerate(np.asarray(rows)):
            order = row[::-1].copy() if reverse else row
            for k in keys:
                t[k].grad = None
            loss = loss_of(t, order, h)
            loss.backward()
            lr = float(np.float32(learning_rate64(h["lr_policy"], h["lr"], it, h["gamma"], h["power"], h["stepsize"])))
            with torch.no_grad():
                for k in keys:
                    rate = num(np.float32(lr) * np.float32(lm[k])) if f32 else lr * lm[k]
                    decay = num(np.float32(h["weight_decay"]) * np.float32(dm[k])) if f32 else num(h["weight_decay"]) * dm[k]
                    d = t[k].grad + decay * t[k]
                    hist[k] = num(h["momentum"]) * hist[k] + rate * d
                    t[k] -= hist[k]
            losses.append(float(loss.item()))
        return np.array(losses, np.float64), {k: t[k].detach().numpy().copy() for k in keys}


def sgd_trajectory(state, img, lab, rows, dtype, hyper=None, lr_mult=None, decay_mult=None, reverse=False, threads=None):
    """The stock network (no conv ReLUs) under caffe_sgd_trajectory's rule -> (every step's loss f64 [len(rows)], the final state)"""
    def loss_of(t, order, h):
        return _loss(t, np.asarray(img)[order], np.asarray(lab)[order], dtype, h["input_scale"])

    return caffe_sgd_trajectory(state, api.TORCH_KEYS, loss_of, rows, dtype, hyper, lr_mult, decay_mult, reverse, threads)


def sgd_trajectory_yardstick(state, img, lab, rows, hyper=None, lr_mult=None, decay_mult=None):
    """-> (losses64, state64, e32 of every step's loss, {key: e32 of the final state}): the two float32 runs of the same rule"""
    import torch
    l64, s64 = sgd_trajectory(state, img, lab, rows, torch.float64, hyper, lr_mult, decay_mult)
    la, sa = sgd_trajectory(state, img, lab, rows, torch.float32, hyper, lr_mult, decay_mult)
    lb, sb = sgd_trajectory(state, img, lab, rows, torch.float32, hyper, lr_mult, decay_mult, reverse=True, threads=1)
    e32 = {k: max(float(np.abs(sa[k].astype(np.float64) - s64[k]).max()), float(np.abs(sb[k].astype(np.float64) - s64[k]).max())) for k in api.TORCH_KEYS}
    return l64, s64, np.maximum(np.abs(la - l64), np.abs(lb - l64)), e32


def recipe(hyper=None, lr_mult=None, decay_mult=None):
    """The gpd_train_recipe and the Trainer keywords of a hyper dict like SOLVER -> (recipe, kw)"""
    h = dict(SOLVER, **(hyper or {}))
    r = api.train_default_recipe(1, momentum=h["momentum"], lr_policy=POLICIES[h["lr_policy"]], gamma=h["gamma"], power=h["power"],
                                 stepsize=h["stepsize"], lr_mult=lr_mult or {}, decay_mult=decay_mult or {})
    return r, dict(lr=h["lr"], weight_decay=h["weight_decay"], input_scale=h["input_scale"])
