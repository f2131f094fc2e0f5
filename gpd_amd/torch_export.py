"""python -m gpd_amd.torch_export MODEL.pwf OUT_DIR [--input-scale S]

A state dict saved by the reference's PyTorch training scripts (pytorch/train_net3.py: torch.save(model.state_dict(), ...) of
pytorch/network.py::Net, possibly wrapped in nn.DataParallel) -> a parameter directory for the host layer (HipClassifier,
detect_grasps): the eight tensors raw little-endian float32 IN TORCH LAYOUT — conv1.weight.bin ... fc2.bias.bin — and a
network.cfg that says so (layout = torch), that the network has a ReLU after each convolution (conv_relu = 1) and what its
inputs were multiplied with in training (input_scale, hdf5_dataset.py:17: 1/256).  Nothing is converted here: the re-layout
into what gpd_hip_set_lenet_weights takes lives in one place, gpd_hip_lenet_from_torch of the C library, which the host layer
calls when it finds network.cfg.  From Python: Context.set_lenet_torch(state).

A state dict of another shape of that script family — other layer widths, or NetCCFFF with fc3.* (three dense layers) — is
written as its 8 or 10 tensors, and network.cfg then also names conv1_out, conv2_out, fc1_out and fc2_out: the host layer loads it
through gpd_hip_lenet_net_from_torch / gpd_hip_set_lenet_net (the shape-general route).  From Python: Context.set_lenet_net(state).
"""
import argparse
import os
import sys

import numpy as np

from gpd_amd import api

FILES = {k: k + ".bin" for k in api.TORCH_KEYS}


def _general_net(state):
    """None for the stock network (20 / 50 / 500, two dense layers: the branch of export() below, unchanged), else
    (LenetShape, tensors) of api.torch_net_arrays: other widths, or fc3.* keys (pytorch/network.py::NetCCFFF)."""
    keys = {str(k)[len("module."):] if str(k).startswith("module.") else str(k) for k in state.keys()}
    if "fc3.weight" not in keys and "fc3.bias" not in keys:
        t = api.torch_state_arrays(state)
        if [t[k].size for k in api.TORCH_KEYS[1:]] == [20, 25000, 50, 3600000, 500, 1000, 2]:
            return None
    return api.torch_net_arrays(state)


def _export_general(shape, arrs, out_dir, input_scale, conv_relu=True):
    """The 8 or 10 tensors in torch layout and a network.cfg that also names the widths; the host layer converts them with
    gpd_hip_lenet_net_from_torch and scores on the shape-general route (gpd_hip_set_lenet_net)."""
    if not api.lenet_shape_check(shape):
        raise ValueError("%r is outside the limits of the general route: %s" % (shape, api.lib().gpd_hip_last_error().decode()))
    os.makedirs(out_dir, exist_ok=True)
    names = [k + ".bin" for k in api.TORCH_NET_KEYS[:len(arrs)]]
    for name, a in zip(names, arrs):
        a.astype("<f4").tofile(os.path.join(out_dir, name))
    with open(os.path.join(out_dir, "network.cfg"), "w") as f:
        f.write("# written by gpd_amd.torch_export: pytorch/network.py::%s, tensors as torch stores them\n"
                "layout = torch\nconv_relu = %d\ninput_scale = %s\nconv1_out = %d\nconv2_out = %d\nfc1_out = %d\nfc2_out = %d\n"
                % ("NetCCFFF" if shape.fc2_out else "Net", int(bool(conv_relu)), repr(float(input_scale)), shape.conv1_out, shape.conv2_out, shape.fc1_out, shape.fc2_out))
    return sorted(names) + ["network.cfg"]


def export(state, out_dir, input_scale=1.0 / 256, conv_relu=True):
    """Write the tensors of `state` and network.cfg into out_dir -> the file names.  The stock network (api.torch_state_arrays):
    eight tensors; any other shape of the family, or NetCCFFF (api.torch_net_arrays): eight or ten, and the widths in network.cfg.
    conv_relu = False: the network was trained without the ReLUs behind the convolutions (the trainer's Caffe variant)."""
    general = _general_net(state)
    if general is not None:
        if not (np.isfinite(input_scale) and input_scale > 0):
            raise ValueError("input_scale must be finite and positive")
        return _export_general(general[0], general[1], out_dir, input_scale, conv_relu)
    t = api.torch_state_arrays(state)
    if not (np.isfinite(input_scale) and input_scale > 0):
        raise ValueError("input_scale must be finite and positive")
    if t["conv1.weight"].size % 500 != 0 or t["conv1.weight"].size == 0:
        raise ValueError("conv1.weight is not [20][C][5][5]")
    os.makedirs(out_dir, exist_ok=True)
    for k, name in FILES.items():
        t[k].astype("<f4").tofile(os.path.join(out_dir, name))
    with open(os.path.join(out_dir, "network.cfg"), "w") as f:
        f.write("# written by gpd_amd.torch_export: pytorch/network.py::Net, tensors as torch stores them\n"
                "layout = torch\nconv_relu = %d\ninput_scale = %s\n" % (int(bool(conv_relu)), repr(float(input_scale))))
    return sorted(FILES.values()) + ["network.cfg"]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m gpd_amd.torch_export", description="state dict of the reference's PyTorch network -> parameter directory for the host layer")
    ap.add_argument("model", help="state dict saved by torch.save (model.pwf)")
    ap.add_argument("out_dir")
    ap.add_argument("--input-scale", type=float, default=1.0 / 256, help="what the training data was multiplied with (default 1/256)")
    a = ap.parse_args(argv)
    import torch
    state = torch.load(a.model, map_location="cpu")
    if hasattr(state, "state_dict"):  # a whole module was saved
        state = state.state_dict()
    names = export(state, a.out_dir, a.input_scale)
    print("wrote %s: %s" % (a.out_dir, " ".join(names)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
