"""Networks trained by the reference's PyTorch scripts (pytorch/train_net3.py, network.py::Net), host side: the re-layout
gpd_hip_lenet_from_torch, api.lenet_from_torch and the export tool.  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import lenet_torch_ref as ltr
from gpd_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _from_torch(C, scale, st):
    L = api.lib()
    L.gpd_hip_lenet_from_torch.argtypes = [ctypes.c_int, ctypes.c_double] + [ctypes.c_void_p] * 6
    c1, f1, f2 = np.zeros(20 * C * 25, np.float32), np.zeros(7200 * 500, np.float32), np.zeros(1000, np.float32)
    rc = L.gpd_hip_lenet_from_torch(C, scale, _p(st["conv1.weight"]), _p(st["fc1.weight"]), _p(st["fc2.weight"]), _p(c1), _p(f1), _p(f2))
    return rc, c1, f1, f2


@pytest.mark.parametrize("C", [15, 12, 3, 1])
def test_from_torch_is_the_numpy_permutation(C):
    rng = np.random.RandomState(C)
    st = {"conv1.weight": rng.randn(20, C, 5, 5).astype(np.float32), "fc1.weight": rng.randn(500, 7200).astype(np.float32),
          "fc2.weight": rng.randn(2, 500).astype(np.float32)}
    rc, c1, f1, f2 = _from_torch(C, 1.0 / 256, st)
    assert rc == 0
    assert np.array_equal(c1, st["conv1.weight"].reshape(-1) * np.float32(2.0 ** -8))
    # ip1[(p * 50 + c) * 500 + u] = fc1[u][c * 144 + p]
    assert np.array_equal(f1.reshape(144, 50, 500), st["fc1.weight"].reshape(500, 50, 144).transpose(2, 1, 0))
    # ip2[j * 2 + u] = fc2[u][j]
    assert np.array_equal(f2.reshape(500, 2), st["fc2.weight"].T)
    # a scale that is no power of two: one rounding from the double product
    rc, c1, _, _ = _from_torch(C, 0.3, st)
    assert rc == 0 and np.array_equal(c1, (st["conv1.weight"].reshape(-1).astype(np.float64) * 0.3).astype(np.float32))


def test_from_torch_undoes_the_test_relayout():
    w = synth.lenet_weights(3, trained_magnitude=True)
    got = api.lenet_from_torch(ltr.to_torch_layout(w, 3), 3)
    assert sorted(got) == sorted(w)
    for k in w:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], w[k]), k


def test_from_torch_error_returns():
    st = {"conv1.weight": np.zeros((20, 3, 5, 5), np.float32), "fc1.weight": np.zeros((500, 7200), np.float32),
          "fc2.weight": np.zeros((2, 500), np.float32)}
    assert _from_torch(3, 1.0 / 256, st)[0] == 0
    L = api.lib()
    for C in (0, 2, 4, 16, -1):
        out = np.zeros(7200 * 500, np.float32)
        assert L.gpd_hip_lenet_from_torch(C, 1.0 / 256, _p(st["conv1.weight"]), _p(st["fc1.weight"]), _p(st["fc2.weight"]), _p(out), _p(out), _p(out)) == -1
        assert b"channels" in L.gpd_hip_last_error()
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        assert _from_torch(3, scale, st)[0] == -1
        assert b"input_scale" in api.lib().gpd_hip_last_error()
    out = np.zeros(7200 * 500, np.float32)
    a = [_p(st["conv1.weight"]), _p(st["fc1.weight"]), _p(st["fc2.weight"])] + [_p(out)] * 3
    for i in range(6):
        b = list(a)
        b[i] = None
        assert L.gpd_hip_lenet_from_torch(3, 1.0 / 256, *b) == -1
        assert b"null" in L.gpd_hip_last_error()
    with pytest.raises(api.GpdHipError):
        api.lenet_from_torch(ltr.state(3), 3, input_scale=0.0)
    with pytest.raises(ValueError):
        api.lenet_from_torch(ltr.state(3), 15)  # conv1.weight of another channel count
    with pytest.raises(KeyError):
        api.lenet_from_torch({k: v for k, v in ltr.state(3).items() if k != "fc2.bias"}, 3)
    # the flag's own argument check comes before the context is touched
    L.gpd_hip_set_lenet_conv_relu.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert L.gpd_hip_set_lenet_conv_relu(None, 1) == -1
    not_a_context = ctypes.create_string_buffer(4096)
    assert L.gpd_hip_set_lenet_conv_relu(not_a_context, 2) == -1 and L.gpd_hip_set_lenet_conv_relu(not_a_context, -1) == -1


@pytest.mark.parametrize("C", [15, 3])
def test_converted_weights_score_like_torch_without_the_conv_relus(C, oracle_mod):
    """The layouts end to end, without a GPU: the oracle's EigenClassifier on the converted weights and RAW images against the
    float64 torch forward of Net with its two conv ReLUs taken out, on image / 256.  1e-4 is the project's score contract
    (SURVEY 9); a layout mistake is orders of magnitude off."""
    import torch
    n = 6
    img = ltr.images(C)[:n]
    w = api.lenet_from_torch(ltr.state(C), C, 1.0 / 256)
    got = oracle_mod.lenet(img, w)
    want = ltr.forward(ltr.state(C), img, torch.float64, conv_relu=False)["score"]
    err = float(np.abs(got - want).max())
    print("C = %d: max |oracle.lenet(converted) - torch f64 without conv ReLUs| = %.3g" % (C, err))
    assert err <= 1e-4
    # ... and the test's own chain composition is the oracle, bit for bit, when it leaves the ReLUs out too
    sc = np.array([ltr.chain_image(oracle_mod, w, im, conv_relu=False)[2] for im in img[:2]], np.float32)
    assert np.array_equal(sc, got[:2])


def test_api_takes_numpy_torch_and_dataparallel_keys():
    import torch
    st = ltr.state(3)
    want = api.lenet_from_torch(st, 3)
    as_torch = {k: torch.from_numpy(v.copy()).requires_grad_(k.endswith("weight")) for k, v in st.items()}
    prefixed = {"module." + k: v for k, v in as_torch.items()}
    f64 = {k: v.astype(np.float64) for k, v in st.items()}
    for other in (as_torch, prefixed, f64):
        got = api.lenet_from_torch(other, 3)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
    # api.py itself does not import torch
    src = open(os.path.join(ROOT, "gpd_amd", "api.py")).read()
    assert "import torch" not in src and "from torch" not in src
    out = subprocess.run([sys.executable, "-c", "import sys; from gpd_amd import api; assert 'torch' not in sys.modules"], cwd=ROOT)
    assert out.returncode == 0


def test_torch_export_round_trip(tmp_path):
    import torch
    st = ltr.state(3)
    model = tmp_path / "model.pwf"
    torch.save({"module." + k: torch.from_numpy(v.copy()) for k, v in st.items()}, str(model))
    out_dir = tmp_path / "params"
    run = subprocess.run([sys.executable, "-m", "gpd_amd.torch_export", str(model), str(out_dir), "--input-scale", "0.00390625"],
                         cwd=ROOT, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    names = sorted(os.listdir(str(out_dir)))
    assert names == sorted([k + ".bin" for k in st] + ["network.cfg"])
    for k, v in st.items():  # torch layout, untouched
        assert np.array_equal(np.fromfile(str(out_dir / (k + ".bin")), "<f4"), v.reshape(-1)), k
    cfg = {}
    for line in (out_dir / "network.cfg").read_text().splitlines():
        line = line.split("#")[0].strip()
        if line:
            key, val = [x.strip() for x in line.split("=")]
            cfg[key] = val
    assert cfg["layout"] == "torch" and cfg["conv_relu"] == "1" and float(cfg["input_scale"]) == 1.0 / 256
    # what the host layer does with the directory (gpd_hip_lenet_from_torch on the files) is what the Python path loads
    files = {k: np.fromfile(str(out_dir / (k + ".bin")), "<f4") for k in st}
    got, want = api.lenet_from_torch(files, 3, float(cfg["input_scale"])), api.lenet_from_torch(st, 3)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
