"""train_ref.py's references for trainers of any network of the family (gpd_hip_train_create_net): pytorch/network.py::Net
of any widths and ::NetCCFFF with its third dense layer, with the conv ReLUs (Net / NetCCFFF) or without (the Caffe variant).

The keys are those of the state (api.TORCH_KEYS, or api.TORCH_NET_KEYS when fc3.* is there), the flatten is F2 * 144, read off
conv2.weight.  The allowance and the floors are train_ref's: FACTOR = 4 times torch's own float32 error against float64 (the
larger of two float32 runs), 2^-22 * max |g64| per tensor, max(4 |L32 - L64|, 2^-21) for the loss.  Callers do not write into
what they get.

Further down: Caffe's SGD rule on any network of the family (train_caffe_ref's rule, one text), and the inputs of
test_gpu_train_net_edges.py with the condition each stands for, which test_train_net_host.py asserts without a device.
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


# ---- Caffe's SGD rule on any network of the family ---------------------------------------------------------------------------------

def sgd_trajectory(state, img, lab, rows, dtype, hyper=None, lr_mult=None, decay_mult=None, reverse=False, threads=None, conv_relu=False):
    """train_caffe_ref.caffe_sgd_trajectory (Caffe's rule written out, the rate rounded to float32 first; NOT torch.optim.SGD)
    over keys_of(state) and the general _forward; conv_relu False is the Caffe network the recipe trains -> (every step's loss
    f64 [len(rows)], the final state {key: numpy of dtype})"""
    import train_caffe_ref as cr

    def loss_of(t, order, h):
        return _net_loss(t, np.asarray(img)[order], np.asarray(lab)[order], dtype, h["input_scale"], conv_relu)

    return cr.caffe_sgd_trajectory(state, keys_of(state), loss_of, rows, dtype, hyper, lr_mult, decay_mult, reverse, threads)


def sgd_trajectory_yardstick(state, img, lab, rows, hyper=None, lr_mult=None, decay_mult=None, conv_relu=False):
    """-> (losses64, state64, e32 of every step's loss, {key: e32 of the final state}): the two float32 runs of the same rule"""
    l64, s64 = sgd_trajectory(state, img, lab, rows, torch.float64, hyper, lr_mult, decay_mult, conv_relu=conv_relu)
    la, sa = sgd_trajectory(state, img, lab, rows, torch.float32, hyper, lr_mult, decay_mult, conv_relu=conv_relu)
    lb, sb = sgd_trajectory(state, img, lab, rows, torch.float32, hyper, lr_mult, decay_mult, reverse=True, threads=1, conv_relu=conv_relu)
    e32 = {k: max(float(np.abs(sa[k].astype(np.float64) - s64[k]).max()), float(np.abs(sb[k].astype(np.float64) - s64[k]).max())) for k in s64}
    return l64, s64, np.maximum(np.abs(la - l64), np.abs(lb - l64)), e32


def xavier_state(C, shape, seed=1, bias=0.1):
    """train_caffe_ref.xavier_state at other widths: init_xavier with the biases set to +-bias in turn (a zero bias leaves
    every all-zero window a four-way tie at 0) -> a fresh dict"""
    st = api.init_xavier(C, seed, shape=shape)
    for k in st:
        if k.endswith("bias"):
            st[k][:] = bias * (1 - 2 * (np.arange(st[k].size) % 2))
    return st


# ---- the inputs of test_gpu_train_net_edges.py, with the condition each stands for asserted on the float64 reference ---------------
# (shared with test_train_net_host.py, which asserts the same conditions where there is no device)

SGD_FROZEN = ("conv1.weight", "conv2.bias", "fc2.weight")   # each between two tensors that move: a slot boundary one off shows on both sides
SGD_BIASES = ("conv1.bias", "conv2.bias", "fc1.bias", "fc2.bias")
# case -> (widths, the step policy?, lr_mult, decay_mult)
SGD_CASES = {"ccfff inv": ((6, 16, 120, 84), False, None, None), "ccfff step": ((6, 16, 120, 84), True, None, None),
             "frozen": ((7, 9, 33), False, dict.fromkeys(SGD_FROZEN, 0.0), None),
             "no bias decay": ((7, 9, 33), False, None, dict.fromkeys(SGD_BIASES, 0.0))}


def sgd_case(case):
    """-> (widths, state, images, labels, rows, hyper, lr_mult, decay_mult): C = 3, test_gpu_train_caffe's six rows of five from 20 images"""
    import train_ref
    from test_gpu_train_caffe import N_SET, ROWS, STEP_HYPER
    widths, step, lr_mult, decay_mult = SGD_CASES[case]
    lab = train_ref.labels()[:N_SET]
    assert len({tuple(lab[r].tolist()) for r in ROWS}) == len(ROWS)  # the labels differ from row to row: a wrong row shows
    return widths, xavier_state(3, widths), train_ref.images(3)[:N_SET], lab, ROWS, (STEP_HYPER if step else {}), lr_mult, decay_mult


def check_sgd_moves(case, st0, s64, lr_mult):
    """The condition of an SGD case on its float64 reference: a frozen tensor stands still, every other one (fc3.* among them)
    moves by more than 1e-5, so that its update is observed -> {key: moved by}"""
    moved = {k: float(np.abs(s64[k] - st0[k]).max()) for k in s64}
    for k, m in moved.items():
        if lr_mult and k in lr_mult:
            assert m == 0, (case, k, m)
        else:
            assert m > 1e-5, (case, k, m)
    return moved


BATCH_DIMS = (1, 3, 5, 33, 9)                       # widths that are no multiple of 2, 8 or 32
BATCH_EDGES = (7, 8, 9, 31, 32, 33, 63, 65, 257)    # around the chains of 8, the 32-row tiles, head_kernel's 64-image blocks, block_sum's 256
BATCH_SEED = 2


def batch_indices(B, n):
    """The last B of n images, the first half of the list reversed (test_gpu_train_net's order)"""
    idx = (n - 1 - np.arange(B)).astype(np.int32)
    idx[: B // 2] = idx[: B // 2][::-1]
    return idx


def part_terms(dims):
    """The three per-image sizes whose largest sizes the trainer's partial buffer: conv2's dW partial, conv1's four, fc1's 16 splits"""
    Cn, F1, F2, H1, _ = dims
    return F2 * F1 * 25, 4 * F1 * 25 * Cn, 16 * H1


PART_DIMS = ((1, 1, 1, 1024, 0), (1, 2, 3, 1000, 7))  # 16 H1 decides
DEAD_DIMS = (3, 6, 16, 120, 84)
DEAD_SEED = 2
DEAD_IDX = np.array([69, 3, 41, 17, 8], np.int32)


def dead_state(layer, live=None):
    """init_state(3, DEAD_SEED) of DEAD_DIMS with `layer`.bias = -1000: every unit of that dense layer is clamped on every
    image; live = u: unit u alone keeps a bias of 1 -> a fresh dict"""
    st = api.init_state(DEAD_DIMS[0], DEAD_SEED, shape=DEAD_DIMS[1:])
    st[layer + ".bias"][:] = -1000.0
    if live is not None:
        st[layer + ".bias"][live] = 1.0
    return st


# which gradients a dead layer leaves: the biases behind it, and the weights whose input is not all zero
DEAD_NONZERO = {"fc2": ("fc3.bias",), "fc1": ("fc2.bias", "fc3.weight", "fc3.bias")}


def check_dead_reference(layer, live, g64):
    """The condition of a dead / nearly dead layer on the float64 gradients"""
    if live is None:
        for k, g in g64.items():
            assert (np.abs(g).max() > 0) == (k in DEAD_NONZERO[layer]), (layer, k, float(np.abs(g).max()))
    else:
        assert all(np.abs(g).max() > 0 for g in g64.values()), {k: float(np.abs(g).max()) for k, g in g64.items()}
        rows = np.flatnonzero(np.abs(g64[layer + ".weight"]).max(axis=1) > 0)
        assert rows.tolist() == [live], (layer, rows)
        assert np.flatnonzero(g64[layer + ".bias"]).tolist() == [live]


HEAD_DIMS = (3, 6, 16, 120, 84)
HEAD_SEED = 2
HEAD_B = 16


def _head_margins0():
    import train_ref
    st = api.init_state(HEAD_DIMS[0], HEAD_SEED, shape=HEAD_DIMS[1:])
    z = logits(st, train_ref.images(HEAD_DIMS[0])[:HEAD_B], torch.float64)
    return st, z[:, 1] - z[:, 0]


def _scaled_head(st, a, centre):
    """st with fc3 scaled by a and fc3.bias[1] moved so that d = a * (d0 - centre) -> (state, float64 margins d)"""
    import train_ref
    st = {k: np.array(v) for k, v in st.items()}
    st["fc3.weight"] = (st["fc3.weight"].astype(np.float64) * a).astype(np.float32)
    b = st["fc3.bias"].astype(np.float64) * a
    b[1] -= a * centre
    st["fc3.bias"] = b.astype(np.float32)
    z = logits(st, train_ref.images(HEAD_DIMS[0])[:HEAD_B], torch.float64)
    return st, z[:, 1] - z[:, 0]


def both_branches_state():
    """test_gpu_train_edges.test_both_head_branches_in_one_batch on NetCCFFF: the third largest |d0 - median| on 1.5, with the
    conditions on the margins asserted -> (state, margins)"""
    import train_ref
    lab = train_ref.labels()[:HEAD_B]
    st0, d0 = _head_margins0()
    centre = float(np.median(d0))
    st, d = _scaled_head(st0, 1.5 / float(np.sort(np.abs(d0 - centre))[-3]), centre)
    inner, outer = np.abs(d) < 0.9, np.abs(d) > 1.1
    assert inner.sum() >= 2 and outer.sum() >= 2 and (d > 0).any() and (d < 0).any(), d
    for side in (inner, outer):
        assert set(lab[side].tolist()) == {0, 1}, (d, lab)
    return st, d


def saturated_state():
    """test_gpu_train_edges.test_saturated_batch on NetCCFFF: every |d| > 50, both signs, a wrong-class image of each label"""
    import train_ref
    lab = train_ref.labels()[:HEAD_B]
    st0, d0 = _head_margins0()
    s = np.sort(d0)
    best = None
    for lo, hi in zip(s[:-1], s[1:]):
        c = 0.5 * (lo + hi)
        if ((lab == 1) & (d0 < c)).any() and ((lab == 0) & (d0 > c)).any() and (best is None or hi - lo > best[1]):
            best = (c, hi - lo)
    assert best is not None
    st, d = _scaled_head(st0, 110.0 / best[1], best[0])
    assert (np.abs(d) > 50).all() and ((lab == 1) & (d < 0)).any() and ((lab == 0) & (d > 0)).any(), d
    return st, d


def eval_state():
    """init_state(3, 2) of HEAD_DIMS with fc3.bias[1] moved by the median margin of train_ref.images(3): an untrained network
    predicts one class for every image, and a count of correct predictions then says nothing -> (state, logits64, e32 of a logit)"""
    import train_ref
    img = train_ref.images(HEAD_DIMS[0])
    st = api.init_state(HEAD_DIMS[0], HEAD_SEED, shape=HEAD_DIMS[1:])
    z = logits(st, img, torch.float64)
    st["fc3.bias"][1] -= np.float32(np.median(z[:, 1] - z[:, 0]))
    z64, e32, _ = logits_e32(st, img)
    d = z64[:, 1] - z64[:, 0]
    # both classes are predicted, and no prediction hangs on the rounding of a float32 forward pass
    assert min((d > 0).sum(), (d < 0).sum()) >= 20 and np.abs(d).min() > 16 * e32, (np.sort(np.abs(d))[:3], e32)
    return st, z64, e32


def logits_e32(state, img, input_scale=1.0 / 256, conv_relu=True):
    """-> (logits64 [n, 2], e32 of either logit, e32 of z1 - z0): the float32 forward in order on several threads, reversed on one"""
    z64 = logits(state, img, torch.float64, input_scale, conv_relu)
    a = logits(state, img, torch.float32, input_scale, conv_relu).astype(np.float64)
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        b = logits(state, np.asarray(img)[::-1], torch.float32, input_scale, conv_relu).astype(np.float64)[::-1]
    finally:
        torch.set_num_threads(before)
    d64 = z64[:, 1] - z64[:, 0]
    return z64, max(float(np.abs(z - z64).max()) for z in (a, b)), max(float(np.abs((z[:, 1] - z[:, 0]) - d64).max()) for z in (a, b))
