"""Inputs and references for the tests of the shape-general LeNet route (gpd_hip_set_lenet_net): the network family of the
reference's pytorch/network.py — C -> F1 -> F2 -> H1 [-> H2] -> 2 on image / 256, Net (H2 = 0) and NetCCFFF (H2 > 0).

  * state(name): seeded weights in torch layout, N(0, gain^2 / fan_in) per layer; the gains and the (negative) conv biases are
    chosen so that scores are O(1) and every ReLU clamps a fair share of its inputs (test_lenet_net.py asserts both as
    conditions on the weights); a second set has the conv weights and biases negated;
  * images(name, n): the images of lenet_torch_ref.images(C), repeated with period 35 when n > 35;
  * forward(): a functional torch forward of the family in float64 (the truth) or float32 — its own text;
  * chain_image(): the network as k-ascending f32 fmaf chains out of oracle.conv_generic for any shape; a dense layer is a
    1x1 "convolution" over [K][1][1], whose chain runs over the K input channels in ascending order.  This is what the device
    route computes bit for bit;
  * EDGE_SHAPES: four shapes at the edges of the route's tiling, with seeds of their own (EDGE_SEEDS); state(), images(),
    route_arrays() and chain() take their names like those of SHAPES;
  * hostile_state() / hostile_images() / hostile_chain(): rows of a seeded state rescaled into the subnormal range, up to 2^100,
    over wide spans and to zero, with images of 255s, of zeros and without a zero pixel.

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
# the edges of the route's tiling (tests/test_gpu_lenet_net_edges.py): not in SHAPES, because one-unit networks cannot have O(1)
# scores and a fair clamp share (test_lenet_net.py asserts on these what CAN be asked of them)
EDGE_SHAPES = {"F": (12, 7, 33, 130, 33),    # 12 channels (chunks 8 + 4); conv2 one odd-k chunk; fc1 K % 32 = 16; fc2 K % 4 = 2; logits ld 36
               "G": (3, 9, 1, 1, 1),         # conv2 chunks 8 + 1; every later width 1 (a row of 4 floats holds one)
               "H": (15, 64, 32, 128, 0),    # every width an exact tile multiple: no padding anywhere
               "I": (1, 1, 1, 1, 0)}         # the smallest network the limits admit
# make_state seeds at which the 35 test images get at least 30 distinct chain scores and no activation tensor is all zero
EDGE_SEEDS = {"F": 0, "G": 3, "H": 0, "I": 0}
ALL_SHAPES = dict(SHAPES, **EDGE_SHAPES)
BATCHES = {"A": (1, 2, 3, 35, 67), "B": (1, 2, 3, 35, 67), "C": (1, 3), "D": (1, 2, 3, 35, 67), "E": (1, 3)}
N_REF = {k: min(max(v), ltr.N_IMAGES) for k, v in BATCHES.items()}  # images the references are computed for
N_REF.update({k: ltr.N_IMAGES for k in EDGE_SHAPES})
SEED = 11
# per-layer gain on N(0, 1 / fan_in) and the conv biases as a fraction of the layer's weight scale: inputs are >= 0 (u8 / 256
# with 60 % zeros, then ReLU outputs), so unit-gain zero-mean weights shrink the signal layer by layer, and the max of a 2x2
# pool window is positive more often than not — the gains bring the scores to O(1), the negative biases the clamped share up
GAIN = {"conv1": 3.0, "conv2": 2.0, "fc1": 1.5, "fc2": 1.5, "fc3": 1.5}
CONV_BIAS = {"conv1": -0.35, "conv2": -0.35}


def images(name, n=None):
    base = ltr.images(ALL_SHAPES[name][0])
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
    st = make_state(ALL_SHAPES[name], EDGE_SEEDS[name] if name in EDGE_SEEDS else SEED + sum(ord(c) for c in name))
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
    return ALL_SHAPES[name], out


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
    out = chain_batch(oracle, ALL_SHAPES[name], arrs, images(name, n or N_REF[name]), conv_relu)
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


# ---- the hostile set: magnitudes at which "an MFMA is an fmaf chain" could stop being true -------------------------------------
HOSTILE_SEED = {"F": 5}
# conv1 filters, then (subnormal outputs, wide-span output, zero output, output times 2^30) of conv2 / fc1 / fc2
HOSTILE_ROWS = {"F": dict(c1_sub=0, c1_big=1, c1_span=2, c1_zero=3, c1_lone=4,
                          conv2=((0, 7, 20), 1, 2, 3), fc1=((0, 50, 101), 1, 2, 3), fc2=((0, 11, 30), 1, 2, 3))}
# three depths of the subnormal range (2^-126 .. 2^-149) per layer; the dense layers' inputs reach 2^13 and more (the lone 1e4)
HOSTILE_SUB_SCALE = {"conv2": (2.0 ** -128, 2.0 ** -133, 2.0 ** -139), "fc1": (2.0 ** -139, 2.0 ** -142, 2.0 ** -146),
                     "fc2": (2.0 ** -139, 2.0 ** -142, 2.0 ** -146)}


@functools.lru_cache(maxsize=None)
def hostile_state(name):
    """A seeded state of ALL_SHAPES[name] with rows rescaled (nothing but scalings of make_state's weights, zeros and one 1e4):
      conv1  one filter times 2^-127 with zero bias: subnormal weights after the input scale, subnormal products and sums, a
             subnormal pool1 plane for conv2's f32 loader; one times 2^100 (bias too), undone by 2^-100 on that input channel of
             conv2; one whose weights span e^-12 .. 1 (any reordering of a chain shows); one all zero; one with a lone 1e4;
      conv2, fc1, fc2  outputs scaled into the subnormal range with zero bias (three depths); one with the wide span, one zero,
             one times 2^30 with the next layer's column scaled back by 2^-30.
    test_lenet_net.py asserts what this has to produce (subnormals in every layer, a maximum above 2^90, everything finite)."""
    shape = ALL_SHAPES[name]
    C, F1, F2, H1, H2 = shape
    assert H2 > 0
    rows = HOSTILE_ROWS[name]
    rng = np.random.RandomState(1000 + HOSTILE_SEED[name])
    st = {k: v.copy() for k, v in make_state(shape, HOSTILE_SEED[name]).items()}
    f32 = np.float32

    def span(k):
        return np.exp(rng.uniform(-12, 0, k)).astype(f32)

    c1 = st["conv1.weight"].reshape(F1, C * 25)
    c1[rows["c1_sub"]] *= f32(2.0 ** -127)
    st["conv1.bias"][rows["c1_sub"]] = 0
    c1[rows["c1_big"]] *= f32(2.0 ** 100)
    st["conv1.bias"][rows["c1_big"]] *= f32(2.0 ** 100)
    c1[rows["c1_span"]] *= span(C * 25)
    c1[rows["c1_zero"]] = 0
    c1[rows["c1_lone"]] *= f32(0.01)
    c1[rows["c1_lone"], 77] = 1e4
    st["conv2.weight"][:, rows["c1_big"]] *= f32(2.0 ** -100)
    # (layer, its [out][k] view, the next layer's weight and how one of ITS input columns is addressed)
    c2 = st["conv2.weight"].reshape(F2, F1 * 25)
    f1 = st["fc1.weight"]                       # [H1][F2 * 144], k = c * 144 + p
    f2 = st["fc2.weight"]                       # [H2][H1]
    f3 = st["fc3.weight"]                       # [2][H2]
    layers = (("conv2", c2, lambda o: f1.reshape(H1, F2, 144)[:, o, :]), ("fc1", f1, lambda o: f2[:, o]), ("fc2", f2, lambda o: f3[:, o]))
    for layer, w, next_col in layers:
        subs, wide, zero, big = rows[layer]
        for o, sc in zip(subs, HOSTILE_SUB_SCALE[layer]):
            w[o] *= f32(sc)
            st[layer + ".bias"][o] = 0
        w[wide] *= span(w.shape[1])
        w[zero] = 0
        w[big] *= f32(2.0 ** 30)
        st[layer + ".bias"][big] *= f32(2.0 ** 30)
        next_col(big)[...] *= f32(2.0 ** -30)
    for v in st.values():
        assert np.isfinite(v).all()
        v.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def hostile_images(name):
    """Twelve of the seeded images, one all 255, one all 0, one dense random without a zero pixel (the u8 loader skips no step)"""
    C = ALL_SHAPES[name][0]
    rng = np.random.RandomState(77)
    img = np.concatenate([images(name, 12), np.full((1, 60, 60, C), 255, np.uint8), np.zeros((1, 60, 60, C), np.uint8),
                          rng.randint(1, 256, (1, 60, 60, C)).astype(np.uint8)])
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def hostile_chain(name, conv_relu=True):
    import oracle
    out = chain_batch(oracle, ALL_SHAPES[name], numpy_route_arrays(hostile_state(name)), hostile_images(name), conv_relu)
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


def subnormals(a):
    """How many values of an f32 array are non-zero and below the smallest normal number"""
    a = np.abs(np.asarray(a, np.float32))
    return int(((a > 0) & (a < np.float32(2.0 ** -126))).sum())
