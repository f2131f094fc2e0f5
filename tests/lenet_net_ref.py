"""Inputs and references for the tests of the shape-general LeNet route (gpd_hip_set_lenet_net): the network family of the
reference's pytorch/network.py — C -> F1 -> F2 -> H1 [-> H2] -> 2 on image / 256, Net (H2 = 0) and NetCCFFF (H2 > 0).

  * state(name): seeded weights in torch layout, N(0, gain^2 / fan_in) per layer; the gains and the (negative) conv biases are
    chosen so that scores are O(1) and every ReLU clamps a fair share of its inputs (test_lenet_net.py asserts both as
    conditions on the weights); a second set has the conv weights and biases negated;
  * images(name, n): the images of lenet_torch_ref.images(C), repeated with period 35 when n > 35;
  * forward(): a functional torch forward of the family in float64 (the truth) or float32 — its own text;
  * chain_image(): the network as k-ascending f32 fmaf chains out of oracle.conv_generic for any shape; a dense layer is a
    1x1 "convolution" over [K][1][1], whose chain runs over the K input channels in ascending order.  This is what the device
    route computes bit for bit.

Everything is computed once per key and shared (lru_cache); callers do not write into what they get.
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import lenet_torch_ref as ltr

INPUT_SCALE = 1.0 / 256
# name -> (channels, conv1_out, conv2_out, fc1_out, fc2_out)
SHAPES = {"A": (3, 6, 16, 120, 84),          # the reference's NetCCFFF line; every width under one tile
          "B": (1, 33, 17, 65, 0),           # one past a 32-tile and a 64-tile edge, odd K
          "C": (15, 40, 100, 500, 0),        # the reference's wide Net
          "D": (15, 20, 50, 500, 0),         # the stock shape
          "E": (1, 64, 128, 1024, 1024)}     # every upper limit
BATCHES = {"A": (1, 2, 3, 35, 67), "B": (1, 2, 3, 35, 67), "C": (1, 3), "D": (1, 2, 3, 35, 67), "E": (1, 3)}
N_REF = {k: min(max(v), ltr.N_IMAGES) for k, v in BATCHES.items()}  # images the references are computed for
SEED = 11
# per-layer gain on N(0, 1 / fan_in) and the conv biases as a fraction of the layer's weight scale: inputs are >= 0 (u8 / 256
# with 60 % zeros, then ReLU outputs), so unit-gain zero-mean weights shrink the signal layer by layer, and the max of a 2x2
# pool window is positive more often than not — the gains bring the scores to O(1), the negative biases the clamped share up
GAIN = {"conv1": 3.0, "conv2": 2.0, "fc1": 1.5, "fc2": 1.5, "fc3": 1.5}
CONV_BIAS = {"conv1": -0.35, "conv2": -0.35}


def images(name, n=None):
    base = ltr.images(SHAPES[name][0])
    if n is None or n <= len(base):
        return base if n is None else base[:n]
    return base[np.arange(n) % len(base)]


def make_state(shape, seed):
    """Seeded weights of any shape of the family, torch layout"""
    C, F1, F2, H1, H2 = shape
    rng = np.random.RandomState(seed)
    dims = [("conv1", (F1, C, 5, 5)), ("conv2", (F2, F1, 5, 5)), ("fc1", (H1, F2 * 144))]
    dims += [("fc2", (H2, H1)), ("fc3", (2, H2))] if H2 else [("fc2", (2, H1))]
    st = {}
    for layer, shp in dims:
        fan_in = int(np.prod(shp[1:]))
        std = GAIN[layer] / np.sqrt(fan_in)
        st[layer + ".weight"] = (rng.randn(*shp) * std).astype(np.float32)
        b = rng.randn(shp[0]) * 0.1
        if layer in CONV_BIAS:
            b = b * 0.25 + CONV_BIAS[layer]
        st[layer + ".bias"] = b.astype(np.float32)
    return st


@functools.lru_cache(maxsize=None)
def state(name, negated=False):
    st = make_state(SHAPES[name], SEED + sum(ord(c) for c in name))
    if negated:
        for k in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias"):
            st[k] = -st[k]
    for v in st.values():
        v.setflags(write=False)
    return st


def forward(st, img, dtype, conv_relu=True, input_scale=INPUT_SCALE):
    """The family's forward, functional -> dict of numpy arrays of `dtype`: pre1 / pre2 (pooled, before the ReLU), pool1, pool2,
    z1, z2 (dense pre-activations; z2 None without fc3), fc1, fc2, logits [n, 2], score [n]"""
    import torch
    import torch.nn.functional as F
    t = {k: torch.from_numpy(np.array(v)).to(dtype) for k, v in st.items()}
    x = torch.from_numpy(np.array(np.transpose(img, (0, 3, 1, 2)), order="C")).to(dtype) * input_scale
    with torch.no_grad():
        pre1 = F.max_pool2d(F.conv2d(x, t["conv1.weight"], t["conv1.bias"]), 2)
        p1 = F.relu(pre1) if conv_relu else pre1
        pre2 = F.max_pool2d(F.conv2d(p1, t["conv2.weight"], t["conv2.bias"]), 2)
        p2 = F.relu(pre2) if conv_relu else pre2
        z1 = F.linear(p2.reshape(len(img), -1), t["fc1.weight"], t["fc1.bias"])  # channel-major flatten, as torch's view()
        a1 = F.relu(z1)
        if "fc3.weight" in t:
            z2 = F.linear(a1, t["fc2.weight"], t["fc2.bias"])
            a2 = F.relu(z2)
            y = F.linear(a2, t["fc3.weight"], t["fc3.bias"])
        else:
            z2 = a2 = None
            y = F.linear(a1, t["fc2.weight"], t["fc2.bias"])
    out = dict(pre1=pre1, pool1=p1, pre2=pre2, pool2=p2, z1=z1, fc1=a1, z2=z2, fc2=a2, logits=y, score=y[:, 1] - y[:, 0])
    return {k: (None if v is None else v.numpy()) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def truth(name, negated=False, dtype="float64", conv_relu=True):
    import torch
    return forward(state(name, negated), images(name, N_REF[name]), getattr(torch, dtype), conv_relu)


@functools.lru_cache(maxsize=None)
def route_arrays(name, negated=False):
    """(shape tuple, the tensors in the route's layouts) by numpy_route_arrays below: the references need none of the code
    under test (test_lenet_net.py holds gpd_hip_lenet_net_from_torch against the same function)"""
    out = numpy_route_arrays(state(name, negated))
    for a in out:
        a.setflags(write=False)
    return SHAPES[name], out


def numpy_route_arrays(st, input_scale=INPUT_SCALE):
    """The same conversion in numpy: what gpd_hip_lenet_net_from_torch must write"""
    F2, H1 = st["conv2.weight"].shape[0], st["fc1.weight"].shape[0]
    out = [(st["conv1.weight"].astype(np.float64) * input_scale).astype(np.float32).ravel(), st["conv1.bias"].ravel(),
           st["conv2.weight"].ravel(), st["conv2.bias"].ravel(),
           # out[(p * F2 + c) * H1 + u] = fc1[u][c * 144 + p]
           np.ascontiguousarray(st["fc1.weight"].reshape(H1, F2, 144).transpose(2, 1, 0)).ravel(), st["fc1.bias"].ravel(),
           np.ascontiguousarray(st["fc2.weight"].T).ravel(), st["fc2.bias"].ravel()]
    if "fc3.weight" in st:
        out += [np.ascontiguousarray(st["fc3.weight"].T).ravel(), st["fc3.bias"].ravel()]
    return out


def _pool(h):
    F, H, W = h.shape
    return h.reshape(F, H // 2, 2, W // 2, 2).max(axis=(2, 4))


def _dense_chain(oracle, x, w_ku, b):
    """x [K], w_ku [K][U] (the route's k-major layout), b [U] -> [U]: one k-ascending chain per unit, then + bias"""
    K, U = w_ku.shape
    w = np.ascontiguousarray(w_ku.T).reshape(U, K, 1, 1)
    return oracle.conv_generic(np.ascontiguousarray(x, np.float32).reshape(K, 1, 1), w, b).reshape(U)


def chain_image(oracle, shape, arrs, img_hwc, conv_relu=True, keep_conv=False):
    """One image through f32 fmaf chains (arrs: the route's layouts) -> dict(pool1 [F1,28,28], pool2 [F2,12,12], fc1 [H1],
    fc2 [H2] or None, logits [2], score); keep_conv: also conv1 / conv2 (pre-pool) and the layer inputs x0 / flat"""
    C, F1, F2, H1, H2 = shape
    zero = np.float32(0)
    x = np.ascontiguousarray(np.transpose(img_hwc, (2, 0, 1)).astype(np.float32))
    c1 = oracle.conv_generic(x, arrs[0].reshape(F1, C, 5, 5), arrs[1])
    p1 = _pool(c1)
    if conv_relu:
        p1 = np.maximum(p1, zero)
    c2 = oracle.conv_generic(p1, arrs[2].reshape(F2, F1, 5, 5), arrs[3])
    p2 = _pool(c2)
    if conv_relu:
        p2 = np.maximum(p2, zero)
    flat = np.ascontiguousarray(p2.reshape(F2, 144).T).reshape(-1)  # j = pixel * F2 + channel
    a1 = np.maximum(_dense_chain(oracle, flat, arrs[4].reshape(F2 * 144, H1), arrs[5]), zero)
    if H2:
        a2 = np.maximum(_dense_chain(oracle, a1, arrs[6].reshape(H1, H2), arrs[7]), zero)
        y = _dense_chain(oracle, a2, arrs[8].reshape(H2, 2), arrs[9])
    else:
        a2 = None
        y = _dense_chain(oracle, a1, arrs[6].reshape(H1, 2), arrs[7])
    out = dict(pool1=p1, pool2=p2, fc1=a1, fc2=a2, logits=y, score=np.float32(y[1] - y[0]))
    if keep_conv:
        out.update(x0=x, conv1=c1, conv2=c2, flat=flat)
    return out


def chain_batch(oracle, shape, arrs, imgs, conv_relu=True):
    """chain_image over a batch -> dict of stacked arrays (the ctypes calls release the interpreter lock)"""
    oracle.lib()
    with ThreadPoolExecutor(8) as pool:
        outs = list(pool.map(lambda im: chain_image(oracle, shape, arrs, im, conv_relu), imgs))
    return {k: (None if outs[0][k] is None else np.stack([o[k] for o in outs])) for k in outs[0]}


@functools.lru_cache(maxsize=None)
def chain(name, negated=False, conv_relu=True, n=None):
    """The first n (default N_REF[name]) images through the chain network; image i of a longer batch is image i % 35 of this"""
    import oracle
    _, arrs = route_arrays(name, negated)
    out = chain_batch(oracle, SHAPES[name], arrs, images(name, n or N_REF[name]), conv_relu)
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out
