"""The shape-general LeNet route, host side: the limits (gpd_hip_lenet_shape_check), the re-layout
(gpd_hip_lenet_net_from_torch, api.torch_net_arrays), the export tool on other shapes and on NetCCFFF — and the yardstick the
device tests use: the fmaf-chain network of lenet_net_ref.py against float64.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import lenet_net_ref as R
import lenet_torch_ref as ltr
from gpd_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(R.SHAPES)
EDGE_NAMES = sorted(R.EDGE_SHAPES)


def test_shape_limits():
    L = api.lib()
    for name in NAMES + EDGE_NAMES:
        assert api.lenet_shape_check(api.LenetShape(*R.ALL_SHAPES[name])), name
    ok = (15, 20, 50, 500, 0)
    assert api.lenet_shape_check(api.LenetShape(*ok))
    for C in (1, 3, 12, 15):
        assert api.lenet_shape_check(api.LenetShape(C, 1, 1, 1, 0))
        assert api.lenet_shape_check(api.LenetShape(C, 64, 128, 1024, 1024))
    bad = [(2, 20, 50, 500, 0), (0, 20, 50, 500, 0), (16, 20, 50, 500, 0),
           (15, 65, 50, 500, 0), (15, 0, 50, 500, 0), (15, 20, 129, 500, 0), (15, 20, 0, 500, 0),
           (15, 20, 50, 1025, 0), (15, 20, 50, 0, 0), (15, 20, 50, 500, 1025), (15, 20, 50, 500, -1)]
    for b in bad:
        assert L.gpd_hip_lenet_shape_check(ctypes.byref(api.LenetShape(*b))) == -1, b
        assert b"limits" in L.gpd_hip_last_error()
    assert L.gpd_hip_lenet_shape_check(None) == -1 and b"null" in L.gpd_hip_last_error()
    # the other host-only entry refuses null pointers and bad shapes before it reads anything
    sh = api.LenetShape(*ok)
    table = (ctypes.c_void_p * 10)()
    assert L.gpd_hip_lenet_net_from_torch(None, 1.0 / 256, table, table) == -1
    assert L.gpd_hip_lenet_net_from_torch(ctypes.byref(sh), 1.0 / 256, None, table) == -1
    assert L.gpd_hip_lenet_net_from_torch(ctypes.byref(sh), 1.0 / 256, table, None) == -1
    assert L.gpd_hip_lenet_net_from_torch(ctypes.byref(sh), 1.0 / 256, table, table) == -1 and b"null" in L.gpd_hip_last_error()
    assert L.gpd_hip_lenet_net_from_torch(ctypes.byref(api.LenetShape(*bad[0])), 1.0 / 256, table, table) == -1


@pytest.mark.parametrize("name", ["A", "B"])
def test_net_from_torch_is_the_numpy_permutation(name):
    st = R.state(name)
    shape, got = api.lenet_net_from_torch(st, 1.0 / 256)
    assert shape.as_tuple() == R.SHAPES[name]
    want = R.numpy_route_arrays(st)
    assert len(got) == len(want) == (10 if R.SHAPES[name][4] else 8)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float32 and np.array_equal(g, w), i
    assert np.array_equal(got[0], st["conv1.weight"].ravel() * np.float32(2.0 ** -8))
    # a scale that is no power of two: one rounding from the double product
    _, got = api.lenet_net_from_torch(st, 0.3)
    assert np.array_equal(got[0], (st["conv1.weight"].ravel().astype(np.float64) * 0.3).astype(np.float32))
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(api.GpdHipError, match="input_scale"):
            api.lenet_net_from_torch(st, scale)


def test_stock_shape_conversion_is_lenet_from_torch():
    """At the stock shape the route's layouts are the Eigen layouts of gpd_hip_lenet_from_torch"""
    st = ltr.state(3)
    shape, got = api.lenet_net_from_torch(st)
    assert shape.as_tuple() == (3, 20, 50, 500, 0)
    want = api.lenet_from_torch(st, 3)
    for g, k in zip(got, ("c1w", "c1b", "c2w", "c2b", "f1w", "f1b", "f2w", "f2b")):
        assert np.array_equal(g, want[k].ravel()), k


def test_torch_net_arrays():
    import torch
    for name in ("A", "B"):  # NetCCFFF, Net
        st = R.state(name)
        shape, want = api.torch_net_arrays(st)
        assert shape.as_tuple() == R.SHAPES[name] and len(want) == (10 if shape.fc2_out else 8)
        as_torch = {k: torch.from_numpy(v.copy()).requires_grad_(k.endswith("weight")) for k, v in st.items()}
        prefixed = {"module." + k: v for k, v in as_torch.items()}
        f64 = {k: v.astype(np.float64) for k, v in st.items()}
        for other in (as_torch, prefixed, f64):
            sh, got = api.torch_net_arrays(other)
            assert sh.as_tuple() == shape.as_tuple()
            for g, w in zip(got, want):
                assert g.dtype == np.float32 and g.flags["C_CONTIGUOUS"] and np.array_equal(g, w)
    st = dict(R.state("A"))
    with pytest.raises(KeyError):
        api.torch_net_arrays({k: v for k, v in st.items() if k != "fc3.bias"})
    with pytest.raises(KeyError):
        api.torch_net_arrays({k: v for k, v in st.items() if k != "conv2.bias"})
    for key, shp in (("fc1.weight", (120, 16 * 144 + 1)), ("conv2.weight", (16, 5, 5, 5)), ("fc3.weight", (2, 83)), ("fc2.bias", (85,)),
                     ("conv1.weight", (6, 3, 3, 3)), ("fc2.weight", (84 * 120,))):
        with pytest.raises(ValueError):
            api.torch_net_arrays(dict(st, **{key: np.zeros(shp, np.float32)}))
    # without the fc3 keys the same tensors are no Net: fc2 would have to be [2][120]
    with pytest.raises(ValueError):
        api.torch_net_arrays({k: v for k, v in st.items() if not k.startswith("fc3")})
    # the stock helpers keep their errors
    with pytest.raises(ValueError):
        api.lenet_from_torch(R.state("B"), 1)


def _read_cfg(path):
    cfg = {}
    for line in open(path).read().splitlines():
        line = line.split("#")[0].strip()
        if line:
            key, val = [x.strip() for x in line.split("=")]
            cfg[key] = val
    return cfg


def test_export_round_trip(tmp_path):
    import torch
    from gpd_amd import torch_export
    st = R.state("A")
    model = tmp_path / "model.pwf"
    torch.save({"module." + k: torch.from_numpy(v.copy()) for k, v in st.items()}, str(model))
    out_dir = tmp_path / "params"
    assert torch_export.main([str(model), str(out_dir)]) == 0
    assert sorted(os.listdir(str(out_dir))) == sorted([k + ".bin" for k in st] + ["network.cfg"]) and len(st) == 10
    for k, v in st.items():  # torch layout, untouched
        assert np.array_equal(np.fromfile(str(out_dir / (k + ".bin")), "<f4"), v.reshape(-1)), k
    cfg = _read_cfg(str(out_dir / "network.cfg"))
    assert cfg["layout"] == "torch" and cfg["conv_relu"] == "1" and float(cfg["input_scale"]) == 1.0 / 256
    assert [int(cfg[k]) for k in ("conv1_out", "conv2_out", "fc1_out", "fc2_out")] == list(R.SHAPES["A"][1:])
    # Net of another width: eight files, fc2_out = 0
    out_b = tmp_path / "params_b"
    names = torch_export.export(R.state("B"), str(out_b), 0.5)
    assert sorted(names) == sorted(os.listdir(str(out_b))) and len(names) == 9
    cfg = _read_cfg(str(out_b / "network.cfg"))
    assert [int(cfg[k]) for k in ("conv1_out", "conv2_out", "fc1_out", "fc2_out")] == list(R.SHAPES["B"][1:]) and float(cfg["input_scale"]) == 0.5
    # a shape outside the limits is not written
    big = dict(R.state("B"), **{"conv1.weight": np.zeros((65, 1, 5, 5), np.float32), "conv1.bias": np.zeros(65, np.float32),
                                "conv2.weight": np.zeros((17, 65, 5, 5), np.float32)})
    with pytest.raises(ValueError, match="limits"):
        torch_export.export(big, str(tmp_path / "params_big"))
    assert not os.path.exists(str(tmp_path / "params_big"))
    # the stock network: the directory this tool has always written — eight tensors, and a network.cfg without the new keys
    out_s = tmp_path / "params_stock"
    stock = ltr.state(3)
    names = torch_export.export(stock, str(out_s))
    assert names == sorted(k + ".bin" for k in stock) + ["network.cfg"] == sorted(os.listdir(str(out_s)))
    for k, v in stock.items():
        assert open(str(out_s / (k + ".bin")), "rb").read() == v.astype("<f4").tobytes(), k
    assert (out_s / "network.cfg").read_text() == ("# written by gpd_amd.torch_export: pytorch/network.py::Net, tensors as torch stores them\n"
                                                   "layout = torch\nconv_relu = 1\ninput_scale = 0.00390625\n")


# ---- the yardstick -----------------------------------------------------------------------------------------------------------
def _gamma(m):
    u = m * 2.0 ** -24
    return u / (1.0 - u)


@pytest.mark.parametrize("name", NAMES + EDGE_NAMES)
def test_chain_layers_are_within_the_chain_bound_of_float64(name, oracle_mod):
    """Per layer, on the chain network's OWN f32 inputs: |chain - float64| <= gamma_{K+1} (sum |w x| + |b|), the standard bound of
    a K-term fmaf chain plus the bias add (K + 1 roundings, u = 2^-24) — derived, not measured."""
    import torch
    import torch.nn.functional as F
    shape = R.ALL_SHAPES[name]
    C, F1, F2, H1, H2 = shape
    _, arrs = R.route_arrays(name)
    o = R.chain_image(oracle_mod, shape, arrs, R.images(name, 1)[0], keep_conv=True)
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))

    def conv_check(x, w, b, got, label):
        K = w[0].size
        with torch.no_grad():
            want = F.conv2d(t64(x)[None], t64(w), t64(b))[0].numpy()
            mag = F.conv2d(t64(np.abs(x))[None], t64(np.abs(w)))[0].numpy() + np.abs(b).astype(np.float64)[:, None, None]
        ratio = float((np.abs(got - want) / (_gamma(K + 1) * mag + 1e-300)).max())
        print("%s %s: K = %d, max |chain - f64| / bound = %.3f" % (name, label, K, ratio))
        assert ratio <= 1.0, (label, ratio)

    def dense_check(x, w_ku, b, got, label):
        K = w_ku.shape[0]
        want = x.astype(np.float64) @ w_ku.astype(np.float64) + b
        mag = np.abs(x).astype(np.float64) @ np.abs(w_ku).astype(np.float64) + np.abs(b)
        ratio = float((np.abs(got - want) / (_gamma(K + 1) * mag + 1e-300)).max())
        print("%s %s: K = %d, max |chain - f64| / bound = %.3f" % (name, label, K, ratio))
        assert ratio <= 1.0, (label, ratio)

    conv_check(o["x0"], arrs[0].reshape(F1, C, 5, 5), arrs[1], o["conv1"], "conv1")
    conv_check(o["pool1"], arrs[2].reshape(F2, F1, 5, 5), arrs[3], o["conv2"], "conv2")
    zero = np.float32(0)
    z1 = R._dense_chain(oracle_mod, o["flat"], arrs[4].reshape(F2 * 144, H1), arrs[5])
    assert np.array_equal(np.maximum(z1, zero), o["fc1"])
    dense_check(o["flat"], arrs[4].reshape(F2 * 144, H1), arrs[5], z1, "fc1")
    if H2:
        z2 = R._dense_chain(oracle_mod, o["fc1"], arrs[6].reshape(H1, H2), arrs[7])
        assert np.array_equal(np.maximum(z2, zero), o["fc2"])
        dense_check(o["fc1"], arrs[6].reshape(H1, H2), arrs[7], z2, "fc2")
        dense_check(o["fc2"], arrs[8].reshape(H2, 2), arrs[9], o["logits"], "fc3")
    else:
        dense_check(o["fc1"], arrs[6].reshape(H1, 2), arrs[7], o["logits"], "fc2")


@pytest.mark.parametrize("name", NAMES)
def test_chain_scores_against_float64_and_the_relus_clamp(name):
    """Conditions on the WEIGHTS of lenet_net_ref.py (change gain or seed, not the conditions): the chain network's scores are
    within 2.5e-5 of the float64 torch forward — a quarter of the project's 1e-4 score contract — and every ReLU
    layer sees at least 10 % negative and at least 10 % positive float64 pre-activations."""
    t = R.truth(name)
    for key in ("pre1", "pre2", "z1", "z2"):
        if t[key] is None:
            assert key == "z2" and R.SHAPES[name][4] == 0
            continue
        neg, pos = float((t[key] < 0).mean()), float((t[key] > 0).mean())
        print("%s %s: %.1f %% negative, %.1f %% positive" % (name, key, 100 * neg, 100 * pos))
        assert neg >= 0.10 and pos >= 0.10, (key, neg, pos)
    c = R.chain(name)
    n = R.N_REF[name]
    assert c["score"].shape == (n,) and t["score"].shape == (n,)
    err = float(np.abs(c["score"].astype(np.float64) - t["score"]).max())
    print("%s: %d images, max |chain score - f64| = %.3g, max |score| = %.3g" % (name, n, err, float(np.abs(t["score"]).max())))
    assert err <= 2.5e-5
    assert 0.3 <= float(np.abs(t["score"]).max()) <= 30  # O(1)
    # the chain's clamps are zeros, and the truth's clear negatives are among them
    assert (c["pool1"][t["pre1"] < -1e-3] == 0).all() and (c["pool2"][t["pre2"] < -1e-3] == 0).all() and (c["fc1"][t["z1"] < -1e-3] == 0).all()


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edge_shape_weights_tell_the_images_apart(name):
    """Conditions on the WEIGHTS of the edge shapes (change EDGE_SEEDS, not the conditions): one-unit networks cannot have O(1)
    scores or a fair clamp share, but a test on them says something only if the 35 images get (nearly) 35 different scores and no
    layer is dead — in either conv_relu setting the device tests use."""
    assert not set(R.EDGE_SHAPES) & set(R.SHAPES)
    for relu in (True, False) if name in "FG" else (True,):
        c = R.chain(name, False, relu)
        distinct = len(np.unique(c["score"]))
        live = {k: float((v != 0).mean()) for k, v in c.items() if v is not None}
        print("%s conv_relu = %d: %d distinct scores of %d, non-zero share %s" % (name, relu, distinct, len(c["score"]), live))
        assert len(c["score"]) == 35 and distinct >= 30
        for k, v in c.items():
            assert (v is None) == (k == "fc2" and R.EDGE_SHAPES[name][4] == 0)
            if v is not None:
                assert np.isfinite(v).all() and np.any(v != 0), k
    st, arrs = R.state(name), R.route_arrays(name)[1]
    shape, got = api.lenet_net_from_torch(st, R.INPUT_SCALE)
    assert shape.as_tuple() == R.EDGE_SHAPES[name] and all(np.array_equal(g, w) for g, w in zip(got, arrs))


def test_hostile_set_has_what_it_is_for():
    """Conditions on lenet_net_ref.hostile_state("F") and its images, on the chain reference: everything is finite (NaN is left
    out on purpose: fmaxf and numpy.maximum treat it differently, a question of definition and not of kernels); non-zero
    subnormal values in every layer — at least 100 in pool1, at least 10 in pool2, fc1 and fc2 — with the conv ReLUs on and off;
    a largest magnitude above 2^90; subnormal conv1 weights after the input scale; an image of 255s, one of zeros, one without a
    zero pixel."""
    name = "F"
    st = R.hostile_state(name)
    arrs = R.numpy_route_arrays(st)
    shape, got = api.lenet_net_from_torch(st, R.INPUT_SCALE)  # the library's conversion keeps the subnormal weights
    assert shape.as_tuple() == R.EDGE_SHAPES[name] and all(np.array_equal(g, w) for g, w in zip(got, arrs))
    assert all(np.isfinite(a).all() for a in arrs)
    assert R.subnormals(arrs[0]) >= 250 and all(R.subnormals(arrs[i]) >= 100 for i in (2, 4, 6))
    rows = R.HOSTILE_ROWS[name]
    c1 = arrs[0].reshape(7, 300)
    assert not c1[rows["c1_zero"]].any() and c1[rows["c1_lone"]].max() == np.float32(1e4) * np.float32(2.0 ** -8)
    assert np.abs(c1[rows["c1_big"]]).max() > 2.0 ** 85
    span = np.abs(c1[rows["c1_span"]])
    assert span.max() / span[span > 0].min() > 1e5
    img = R.hostile_images(name)
    assert 12 <= len(img) <= R.ltr.N_IMAGES
    assert (img[-3] == 255).all() and not img[-2].any() and img[-1].min() >= 1
    for relu in (True, False):
        c = R.hostile_chain(name, relu)
        counts = {k: R.subnormals(c[k]) for k in ("pool1", "pool2", "fc1", "fc2")}
        biggest = max(float(np.abs(v).max()) for v in c.values())
        print("hostile F conv_relu = %d: subnormals %s, largest magnitude %.3g, %d distinct scores" % (relu, counts, biggest,
                                                                                                      len(np.unique(c["score"]))))
        for k, v in c.items():
            assert np.isfinite(v).all(), k
        assert counts["pool1"] >= 100 and min(counts["pool2"], counts["fc1"], counts["fc2"]) >= 10
        assert biggest > 2.0 ** 90
        assert len(np.unique(c["score"])) == len(img)
