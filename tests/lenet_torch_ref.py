"""The network of the reference's PyTorch scripts (pytorch/network.py::Net: conv1, ReLU, pool, conv2, ReLU, pool, channel-major
flatten, fc1, ReLU, fc2 on image / 256) for the tests of gpd_hip_set_lenet_conv_relu / gpd_hip_lenet_from_torch, three times:

  * inputs: the images and the state dicts (synth.lenet_weights re-laid into torch layout by numpy here, the inverse of what
    gpd_hip_lenet_from_torch does, conv1 * 256; a second set with conv1 / conv2 weights and biases negated);
  * forward(): a functional torch forward in float64 (the truth) or float32 (the yardstick: the error ONE f32 summation order makes);
  * chain(): the network as k-ascending f32 fmaf chains out of oracle.conv_generic, the same chains as the oracle's convForward —
    what GPD_LENET_F32_CHAIN computes bit for bit.

Everything is computed once per (channels, weight set) and shared (lru_cache); callers do not write into what they get.
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from gpd_amd import synth

N_IMAGES = 35
BATCHES = (1, 2, 3, 35)  # conv kernels: >= 2 images per workgroup; ip2: blocks of 32 images; ip1's X: blocks of 16
INPUT_SCALE = 1.0 / 256
# synth.lenet_weights' default seed (42) leaves one conv2 channel without a clamped value in BOTH weight sets for 15, 12 and 1
# channels (every_channel_clamps below: after the first ReLU pool1 has a large mean, and a conv2 filter can stay positive on it
# with either sign); seed 40 is the nearest below that meets the condition for all four channel counts
WEIGHT_SEED = 40


@functools.lru_cache(maxsize=None)
def images(C):
    rng = np.random.RandomState(7)
    img = rng.randint(0, 256, (N_IMAGES, 60, 60, C)).astype(np.uint8)
    img[rng.rand(N_IMAGES, 60, 60, C) < 0.6] = 0
    img.setflags(write=False)
    return img


def to_torch_layout(w, C):
    """Eigen-layout dict (c1w .. f2b) -> Net's tensors, conv1 * 256 (exact): the inverse of gpd_hip_lenet_from_torch at 1/256"""
    return {"conv1.weight": (w["c1w"].reshape(20, C, 5, 5) * np.float32(256)).astype(np.float32), "conv1.bias": w["c1b"].copy(),
            "conv2.weight": w["c2w"].reshape(50, 20, 5, 5).copy(), "conv2.bias": w["c2b"].copy(),
            # fc1[u][c * 144 + p] = ip1[(p * 50 + c) * 500 + u]
            "fc1.weight": np.ascontiguousarray(w["f1w"].reshape(144, 50, 500).transpose(2, 1, 0)).reshape(500, 7200), "fc1.bias": w["f1b"].copy(),
            "fc2.weight": np.ascontiguousarray(w["f2w"].reshape(500, 2).T), "fc2.bias": w["f2b"].copy()}


@functools.lru_cache(maxsize=None)
def eigen_weights(C, negated=False):
    w = {k: v.copy() for k, v in synth.lenet_weights(C, seed=WEIGHT_SEED, trained_magnitude=True).items()}
    if negated:
        for k in ("c1w", "c1b", "c2w", "c2b"):
            w[k] = -w[k]
    return w


@functools.lru_cache(maxsize=None)
def state(C, negated=False):
    return to_torch_layout(eigen_weights(C, negated), C)


def forward(st, img, dtype, conv_relu=True, input_scale=INPUT_SCALE):
    """Net.forward, functional -> dict(pre1, pool1 [n,20,28,28], pre2, pool2 [n,50,12,12], score [n]) as numpy of `dtype`;
    pre1 / pre2: the pooled values before the ReLU (what it clamps)"""
    import torch
    import torch.nn.functional as F
    t = {k: torch.from_numpy(np.array(v)).to(dtype) for k, v in st.items()}
    x = torch.from_numpy(np.array(np.transpose(img, (0, 3, 1, 2)), order="C")).to(dtype) * input_scale
    with torch.no_grad():
        # (ReLU before or after the 2x2 max-pool is the same function; after it, the clamped values can be looked at)
        pre1 = F.max_pool2d(F.conv2d(x, t["conv1.weight"], t["conv1.bias"]), 2)
        p1 = F.relu(pre1) if conv_relu else pre1
        pre2 = F.max_pool2d(F.conv2d(p1, t["conv2.weight"], t["conv2.bias"]), 2)
        p2 = F.relu(pre2) if conv_relu else pre2
        a1 = F.relu(F.linear(p2.reshape(len(img), 50 * 144), t["fc1.weight"], t["fc1.bias"]))
        y = F.linear(a1, t["fc2.weight"], t["fc2.bias"])
    return dict(pre1=pre1.numpy(), pool1=p1.numpy(), pre2=pre2.numpy(), pool2=p2.numpy(), score=(y[:, 1] - y[:, 0]).numpy())


@functools.lru_cache(maxsize=None)
def truth(C, negated=False, dtype="float64"):
    import torch
    return forward(state(C, negated), images(C), getattr(torch, dtype))


def every_channel_clamps(C):
    """A condition on the INPUTS: every conv1 and conv2 channel has a clamped (negative) pooled value in at least one weight set"""
    a, b = truth(C, False), truth(C, True)
    c1 = (a["pre1"] < 0).any(axis=(0, 2, 3)) | (b["pre1"] < 0).any(axis=(0, 2, 3))
    c2 = (a["pre2"] < 0).any(axis=(0, 2, 3)) | (b["pre2"] < 0).any(axis=(0, 2, 3))
    return bool(c1.all() and c2.all() and len(c1) == 20 and len(c2) == 50)


def _pool(h):
    F, H, W = h.shape
    return h.reshape(F, H // 2, 2, W // 2, 2).max(axis=(2, 4))


def chain_image(oracle, w, img_hwc, conv_relu=True):
    """One image through f32 fmaf chains (w: Eigen layout, conv1 already scaled) -> (pool1 [20,28,28], flat [7200], score)"""
    C = img_hwc.shape[-1]
    x = np.transpose(img_hwc, (2, 0, 1)).astype(np.float32)
    p1 = _pool(oracle.conv_generic(x, w["c1w"].reshape(20, C, 5, 5), w["c1b"]))
    if conv_relu:
        p1 = np.maximum(p1, np.float32(0))
    p2 = _pool(oracle.conv_generic(p1, w["c2w"].reshape(50, 20, 5, 5), w["c2b"]))
    if conv_relu:
        p2 = np.maximum(p2, np.float32(0))
    f = np.ascontiguousarray(p2.reshape(50, 144).T).reshape(7200)  # j = pixel * 50 + channel
    W1 = np.ascontiguousarray(w["f1w"].reshape(7200, 500).T)       # [unit][j]: one output pixel of a 5x5 "convolution" is the j-ascending chain
    a1 = np.maximum(oracle.conv_generic(f.reshape(288, 5, 5), W1.reshape(500, 288, 5, 5), w["f1b"]).reshape(500), np.float32(0))
    W2 = np.ascontiguousarray(w["f2w"].reshape(500, 2).T)
    y = oracle.conv_generic(a1.reshape(20, 5, 5), W2.reshape(2, 20, 5, 5), w["f2b"]).reshape(2)
    return p1, f, np.float32(y[1] - y[0])


def chain_batch(oracle, w, imgs, conv_relu=True):
    """chain_image over a batch, the images side by side (the ctypes calls release the interpreter lock)"""
    oracle.lib()
    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(lambda im: chain_image(oracle, w, im, conv_relu), imgs))


@functools.lru_cache(maxsize=None)
def chain(C, negated=False, n=N_IMAGES):
    """The first n images of images(C) through chain_image on the weights gpd_hip_lenet_from_torch gives -> (pool1 [n,20,28,28], scores [n])"""
    import oracle
    from gpd_amd import api
    w = api.lenet_from_torch(state(C, negated), C, INPUT_SCALE)
    out = chain_batch(oracle, w, images(C)[:n])
    return np.stack([o[0] for o in out]), np.array([o[2] for o in out], np.float32)


def chain_pool1_planes(dev, n):
    """lenet_debug(0) of GPD_LENET_F32_CHAIN, [n][20][784] with a plane's pixels in conv1's chunk order (strips of 8, 8, 8 and 4
    columns, 28 rows each, gpd_amd/csrc/lenet.hip c1_pixel_of) -> [n, 20, 28, 28]"""
    pc = np.arange(784)
    strip, within = pc // 224, pc % 224
    sw = np.where(strip < 3, 8, 4)
    py, px = within // sw, strip * 8 + within % sw
    out = np.zeros((n, 20, 28, 28), np.float32)
    out[:, :, py, px] = dev.reshape(n, 20, 784)
    return out
