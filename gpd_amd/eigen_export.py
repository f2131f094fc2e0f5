"""A state of the Caffe LeNet (the trainer's network 1: no ReLU behind the convolutions) -> a parameter directory in the layout
the reference's EigenClassifier reads (net/eigen_classifier.cpp): conv1_weights.bin [20][25 C], conv1_biases.bin [20],
conv2_weights.bin [50][500], conv2_biases.bin [50], ip1_weights.bin [7200][500], ip1_biases.bin [500], ip2_weights.bin
[500][2], ip2_biases.bin [2], raw little-endian float32 — the arrays gpd_hip_set_lenet_weights takes.  The re-layout is
api.lenet_from_torch (gpd_hip_lenet_from_torch of the C library), with the training input scale folded into conv1 so that raw
0..255 images score the same; nothing is converted here.  No network.cfg is written: a directory without one IS the
reference's format, for the reference's `weights_file` as for this project's host layer.

A network WITH conv ReLUs (pytorch/network.py::Net) cannot be expressed in this format; gpd_amd.torch_export is for it.
"""
import os

import numpy as np

from gpd_amd import api

FILES = dict(c1w="conv1_weights.bin", c1b="conv1_biases.bin", c2w="conv2_weights.bin", c2b="conv2_biases.bin",
             f1w="ip1_weights.bin", f1b="ip1_biases.bin", f2w="ip2_weights.bin", f2b="ip2_biases.bin")


def export(state, out_dir, input_scale=1.0 / 256, conv_relu=False):
    """Write the eight files from `state` (torch layout, see api.torch_state_arrays) into out_dir -> the file names.
    conv_relu: what the caller knows about the state's network; True is refused."""
    if conv_relu:
        raise ValueError("the EigenClassifier format has no ReLU behind the convolutions: a Net state goes through gpd_amd.torch_export")
    if not (np.isfinite(input_scale) and input_scale > 0):
        raise ValueError("input_scale must be finite and positive")
    t = api.torch_state_arrays(state)
    if t["conv1.weight"].size % 500 != 0 or t["conv1.weight"].size == 0:
        raise ValueError("conv1.weight is not [20][C][5][5]")
    w = api.lenet_from_torch(t, t["conv1.weight"].size // 500, input_scale)
    os.makedirs(out_dir, exist_ok=True)
    for k, name in FILES.items():
        np.ascontiguousarray(w[k], "<f4").tofile(os.path.join(out_dir, name))
    return sorted(FILES.values())


def load(directory, fill=None):
    """An Eigen-layout directory -> the c1w .. f2b dict Context.set_lenet_weights takes.  fill: a dict of the same kind that
    supplies the arrays whose files the directory lacks (the reference's snapshot has no ip1_weights.bin)."""
    out = {}
    for k, name in FILES.items():
        path = os.path.join(directory, name)
        if fill is not None and not os.path.exists(path):
            out[k] = np.ascontiguousarray(fill[k], np.float32).ravel()
        else:
            out[k] = np.fromfile(path, "<f4")
    return out


def to_torch(weights, input_scale=1.0 / 256):
    """The inverse of the re-layout, for starting a training run from an Eigen-layout directory (load()): c1w .. f2b -> the
    state in torch layout, conv1 divided by input_scale (exact for a power of two)."""
    c1w = np.asarray(weights["c1w"], np.float32)
    if c1w.size % 500 != 0 or c1w.size == 0:
        raise ValueError("conv1_weights.bin is not [20][25 C]")
    C = c1w.size // 500
    sizes = dict(c1b=20, c2w=25000, c2b=50, f1w=3600000, f1b=500, f2w=1000, f2b=2)
    for k, n in sizes.items():
        if np.asarray(weights[k]).size != n:
            raise ValueError("%s has %d values, %d expected" % (FILES[k], np.asarray(weights[k]).size, n))
    f32 = lambda k: np.asarray(weights[k], np.float32)
    return {"conv1.weight": (c1w.astype(np.float64) / input_scale).astype(np.float32).reshape(20, C, 5, 5),
            "conv1.bias": f32("c1b").reshape(20).copy(),
            "conv2.weight": f32("c2w").reshape(50, 20, 5, 5).copy(), "conv2.bias": f32("c2b").reshape(50).copy(),
            # ip1[(p * 50 + c) * 500 + u] = fc1[u][c * 144 + p]
            "fc1.weight": np.ascontiguousarray(f32("f1w").reshape(144, 50, 500).transpose(2, 1, 0)).reshape(500, 7200),
            "fc1.bias": f32("f1b").reshape(500).copy(),
            "fc2.weight": np.ascontiguousarray(f32("f2w").reshape(500, 2).T), "fc2.bias": f32("f2b").reshape(2).copy()}
