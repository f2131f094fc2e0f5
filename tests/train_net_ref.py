"""train_ref.py's references for trainers of any network of the family (gpd_hip_train_create_net): pytorch/network.py::Net
of any widths and ::NetCCFFF with its third dense layer, with the conv ReLUs (Net / NetCCFFF) or without (the Caffe variant).

The keys are those of the state (api.TORCH_KEYS, or api.TORCH_NET_KEYS when fc3.* is there), the flatten is F2 * 144, read off
conv2.weight.  The allowance and the floors are train_ref's: FACTOR = 4 times torch's own float32 error against float64 (the
larger of two float32 runs), 2^-22 * max |g64| per tensor, max(4 |L32 - L64|, 2^-21) for the loss.  Callers do not write into
what they get.
"""
import numpy as np
import torch  # before anything loads libgpd_hip.so (train_caffe_ref does the same): the process then has one HIP runtime, torch's

from gpd_amd import api
from train_ref import FACTOR, HYPER  # noqa: F401  (re-exported: one statement of each)


def keys_of(state):
    return api.TORCH_NET_KEYS if "fc3.weight" in state else api.TORCH_KEYS


def _forward(t, img, dtype, input_scale, conv_relu):
    import torch.nn.functional as F
    x = torch.from_numpy(np.array(np.transpose(np.asarray(img), (0, 3, 1, 2)), order="C")).to(dtype) * input_scale
    act = F.relu if conv_relu else (lambda v: v)
    h = F.max_pool2d(act(F.conv2d(x, t["conv1.weight"], t["conv1.bias"])), 2)
    h = F.max_pool2d(act(F.conv2d(h, t["conv2.weight"], t["conv2.bias"])), 2)
    h = F.relu(F.linear(h.reshape(len(img), t["conv2.weight"].shape[0] * 144), t["fc1.weight"], t["fc1.bias"]))
    z = F.linear(h, t["fc2.weight"], t["fc2.bias"])
    if "fc3.weight" in t:
        z = F.linear(F.relu(z), t["fc3.weight"], t["fc3.bias"])
    return z


def _net_loss(t, img, lab, dtype, input_scale, conv_relu):
    import torch.nn.functional as F
    y = torch.from_numpy(np.asarray(lab).astype(np.int64))
    return F.cross_entropy(_forward(t, img, dtype, input_scale, conv_relu), y)


def logits(state, img, dtype, input_scale=1.0 / 256, conv_relu=True):
    """The network's logits in `dtype` -> [n, 2]"""
    t = {k: torch.from_numpy(np.array(state[k])).to(dtype) for k in keys_of(state)}
    with torch.no_grad():
        return _forward(t, img, dtype, input_scale, conv_relu).numpy()


def autograd(state, img, lab, dtype, input_scale=1.0 / 256, reverse=False, threads=None, conv_relu=True):
    """-> ({key: gradient as numpy of dtype}, loss)"""
    keys = keys_of(state)
    before = torch.get_num_threads()
    if threads:
        torch.set_num_threads(threads)
    try:
        order = np.arange(len(lab))[::-1].copy() if reverse else np.arange(len(lab))
        t = {k: torch.from_numpy(np.array(state[k])).to(dtype).requires_grad_(True) for k in keys}
        loss = _net_loss(t, np.asarray(img)[order], np.asarray(lab)[order], dtype, input_scale, conv_relu)
        loss.backward()
        return {k: t[k].grad.numpy().copy() for k in keys}, float(loss.item())
    finally:
        torch.set_num_threads(before)


def yardstick(state, img, lab, input_scale=1.0 / 256, conv_relu=True):
    """-> (g64, loss64, {key: e32}, e32 of the loss): e32 = the larger of the two float32 runs' max-abs errors against float64"""
    g64, l64 = autograd(state, img, lab, torch.float64, input_scale, conv_relu=conv_relu)
    a, la = autograd(state, img, lab, torch.float32, input_scale, conv_relu=conv_relu)
    b, lb = autograd(state, img, lab, torch.float32, input_scale, reverse=True, threads=1, conv_relu=conv_relu)
    e32 = {k: max(float(np.abs(a[k].astype(np.float64) - g64[k]).max()), float(np.abs(b[k].astype(np.float64) - g64[k]).max())) for k in g64}
    return g64, l64, e32, max(abs(la - l64), abs(lb - l64))


def check_gradients(what, got, loss, g64, l64, e32, el32):
    """train_ref.check_gradients over the keys of g64: prints every measured ratio before it asserts -> the largest ratio."""
    worst, bad = 0.0, []
    assert set(got) == set(g64), (what, sorted(got), sorted(g64))
    for k in g64:
        assert got[k].shape == g64[k].shape, (what, k, got[k].shape, g64[k].shape)
        err = float(np.abs(got[k].astype(np.float64) - g64[k]).max())
        top = float(np.abs(g64[k]).max())
        allow = max(FACTOR * e32[k], 2.0 ** -22 * top)
        ratio = err / e32[k] if e32[k] > 0 else (0.0 if err == 0 else float("inf"))
        print("%s %-12s max|g64| = %.3g  e32 = %.3g  device error = %.3g  ratio = %.2f  allowance = %.3g" % (what, k, top, e32[k], err, ratio, allow))
        if err > allow:
            bad.append((k, err, allow))
        elif e32[k] > 0 and err > 2.0 ** -22 * top:
            worst = max(worst, ratio)
    lerr, lallow = abs(loss - l64), max(FACTOR * el32, 2.0 ** -21)
    print("%s loss: f64 %.9g  device %.9g  error = %.3g  allowance = %.3g" % (what, l64, loss, lerr, lallow))
    assert not bad, (what, bad)
    assert lerr <= lallow, (what, loss, l64, lallow)
    return worst


def trajectory(state, img, lab, rows, dtype, hyper=None, reverse=False, threads=None, conv_relu=True):
    """The network under torch.optim.Adam(lr, betas, eps, weight_decay): one step per row of `rows` (indices into img / lab;
    reverse: each row back to front) -> (every step's loss f64 [len(rows)], the final state {key: numpy of dtype})"""
    h = dict(HYPER, **(hyper or {}))
    keys = keys_of(state)
    before = torch.get_num_threads()
    if threads:
        torch.set_num_threads(threads)
    try:
        t = {k: torch.from_numpy(np.array(state[k])).to(dtype).requires_grad_(True) for k in keys}
        opt = torch.optim.Adam([t[k] for k in keys], lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=h["weight_decay"])
        losses = []
        for row in np.asarray(rows):
            order = row[::-1].copy() if reverse else row
            opt.zero_grad()
            loss = _net_loss(t, np.asarray(img)[order], np.asarray(lab)[order], dtype, h["input_scale"], conv_relu)
            loss.backward()
            opt.step()
            losses.append(float(loss.item()))
        return np.array(losses, np.float64), {k: t[k].detach().numpy().copy() for k in keys}
    finally:
        torch.set_num_threads(before)


def trajectory_yardstick(state, img, lab, rows, hyper=None, conv_relu=True):
    """-> (losses64, state64, e32 of every step's loss [len(rows)], {key: e32 of the final state}): yardstick()'s two float32 runs"""
    l64, s64 = trajectory(state, img, lab, rows, torch.float64, hyper, conv_relu=conv_relu)
    la, sa = trajectory(state, img, lab, rows, torch.float32, hyper, conv_relu=conv_relu)
    lb, sb = trajectory(state, img, lab, rows, torch.float32, hyper, reverse=True, threads=1, conv_relu=conv_relu)
    e32 = {k: max(float(np.abs(sa[k].astype(np.float64) - s64[k]).max()), float(np.abs(sb[k].astype(np.float64) - s64[k]).max())) for k in s64}
    return l64, s64, np.maximum(np.abs(la - l64), np.abs(lb - l64)), e32
