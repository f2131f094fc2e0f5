"""The host-only half of the Caffe recipe (gpd_train_recipe; no GPU): the learning-rate policies against their
float64 formulas, the refusals of a recipe, the xavier filler, and gpd_amd.eigen_export against api.lenet_from_torch."""
import ctypes as C

import numpy as np
import pytest

import train_caffe_ref as cr
from gpd_amd import api, eigen_export

ITS = (0, 1, 99, 100, 101, 10 ** 4, 2 ** 31)


@pytest.mark.parametrize("policy,kw", [("fixed", {}), ("step", dict(gamma=0.5, stepsize=100)), ("step", dict(gamma=0.1, stepsize=7)),
                                       ("exp", dict(gamma=0.9999)), ("exp", dict(gamma=0.5)), ("inv", dict(gamma=1e-4, power=0.75)),
                                       ("inv", dict(gamma=0.0, power=2.0)), ("inv", dict(gamma=3.0, power=0.5))])
def test_learning_rate_is_the_float64_formula_rounded_once(policy, kw):
    r = api.train_default_recipe(1, lr_policy=cr.POLICIES[policy], **kw)
    for base in (0.01, 1e-3, 0.0):
        for it in ITS:
            want = np.float32(cr.learning_rate64(policy, base, it, kw.get("gamma", 1e-4), kw.get("power", 0.75), kw.get("stepsize", 1)))
            got = api.learning_rate(r, base, it)
            assert got.dtype == np.float32 and got == want, (policy, kw, base, it, got, want)


def test_the_solver_files_schedule():
    r = api.train_default_recipe(1)
    assert (r.network, r.solver, r.momentum, r.lr_policy, r.gamma, r.power) == (1, 1, 0.9, api.LR_INV, 0.0001, 0.75)
    assert list(r.lr_mult) == [1.0] * 8 and list(r.decay_mult) == [1.0] * 8
    assert api.learning_rate(r, api.CAFFE_BASE_LR, 0) == np.float32(0.01)
    assert api.learning_rate(r, api.CAFFE_BASE_LR, 1) < np.float32(0.01)  # inv moves from the second update on
    assert api.learning_rate(r, api.CAFFE_BASE_LR, 9999) == np.float32(0.01 * 1.9999 ** -0.75)
    r0 = api.train_default_recipe(0)
    assert (r0.network, r0.solver, r0.lr_policy) == (0, 0, api.LR_FIXED)
    assert api.learning_rate(r0, 1e-3, 12345) == np.float32(1e-3)


BAD = [dict(network=2), dict(network=-1), dict(solver=2), dict(lr_policy=4), dict(lr_policy=-1), dict(momentum=1.0), dict(momentum=-0.1),
       dict(momentum=float("nan")), dict(lr_policy=1, stepsize=0), dict(gamma=float("inf")), dict(gamma=float("nan")), dict(power=float("nan")),
       dict(power=float("-inf")), dict(lr_policy=3, gamma=-1e-4), dict(lr_mult={"fc1.weight": -1.0}), dict(lr_mult={"conv1.bias": float("nan")}),
       dict(decay_mult={"fc2.bias": float("inf")}), dict(decay_mult={"conv2.weight": -0.5}),
       dict(solver=0, lr_mult={"conv1.weight": 0.0}), dict(solver=0, decay_mult={"fc2.bias": 0.0})]


@pytest.mark.parametrize("kw", BAD, ids=[",".join("%s=%s" % kv for kv in d.items()) for d in BAD])
def test_invalid_recipes_are_refused(kw):
    r = api.train_default_recipe(1, **kw)
    with pytest.raises(api.GpdHipError, match="error -1: .*recipe"):
        api.learning_rate(r, 0.01, 0)
    # ... by create as well, before it looks at anything else: the context here is never touched
    not_a_context = C.create_string_buffer(64)
    out = C.c_void_p()
    p = api.TrainParams()
    api.lib().gpd_hip_train_default_params(C.byref(p))
    assert api.lib().gpd_hip_train_create_recipe(not_a_context, C.byref(p), C.byref(r), C.byref(out)) == -1 and not out.value
    assert b"recipe" in api.lib().gpd_hip_last_error()


def test_learning_rate_and_default_recipe_refuse_their_arguments():
    r = api.train_default_recipe(1)
    for base, it in ((-0.01, 0), (float("nan"), 0), (float("inf"), 0), (0.01, -1)):
        with pytest.raises(api.GpdHipError):
            api.learning_rate(r, base, it)
    with pytest.raises(api.GpdHipError):
        api.train_default_recipe(2)
    # the legal edges: step with stepsize 1, a stepsize below 1 where the policy does not read it, momentum 0
    assert api.learning_rate(api.train_default_recipe(1, lr_policy=1, stepsize=1, gamma=0.5), 1.0, 3) == np.float32(0.125)
    assert api.learning_rate(api.train_default_recipe(1, lr_policy=0, stepsize=0, momentum=0.0), 1.0, 3) == np.float32(1.0)


@pytest.mark.parametrize("C_", [1, 3, 12, 15])
def test_xavier(C_):
    st = api.init_xavier(C_, 7)
    assert [st[k].shape for k in api.TORCH_KEYS] == list(api.torch_state_shapes(C_))
    for k, bound in cr.xavier_bounds(C_).items():
        w = st[k].astype(np.float64)
        assert np.abs(w).max() <= bound, (k, np.abs(w).max(), bound)
        assert w.min() < 0 < w.max()
        if k in ("fc1.weight", "conv2.weight"):  # 3.6 M and 25 000 draws: the top percent of the range is reached
            assert np.abs(w).max() > 0.99 * bound, (k, np.abs(w).max(), bound)
            assert abs(w.mean()) < 0.02 * bound and abs(w.std() - bound / np.sqrt(3.0)) < 0.02 * bound  # uniform, not merely bounded
    for k in api.TORCH_KEYS:
        if k.endswith("bias"):
            assert st[k].tobytes() == bytes(st[k].nbytes)  # +0.0 everywhere
    again, other = api.init_xavier(C_, 7), api.init_xavier(C_, 8)
    for k in api.TORCH_KEYS:
        assert st[k].tobytes() == again[k].tobytes()
        assert k.endswith("bias") or st[k].tobytes() != other[k].tobytes()


@pytest.mark.parametrize("C_", [0, 2, 4, 16, -1])
def test_xavier_refuses_other_channel_counts(C_):
    with pytest.raises(api.GpdHipError, match="channels"):
        api.init_xavier(C_, 0)
    bufs = [np.zeros(4, np.float32) for _ in range(8)]
    ptrs = (C.c_void_p * 8)(*[b.ctypes.data for b in bufs])
    assert api.lib().gpd_hip_train_init_xavier(C_, 0, ptrs) == -1
    assert not any(b.any() for b in bufs)


@pytest.mark.parametrize("C_,scale", [(3, 1.0 / 256), (15, 1.0 / 256), (3, 1.0 / 255)])
def test_export_writes_lenet_from_torch(tmp_path, C_, scale):
    st = api.init_xavier(C_, 3)
    st["conv1.bias"][:] = np.linspace(-1, 1, 20)
    st["fc2.bias"][:] = (0.25, -0.5)
    names = eigen_export.export(st, str(tmp_path / "params"), scale)
    want = api.lenet_from_torch(st, C_, scale)
    sizes = dict(c1w=500 * C_, c1b=20, c2w=25000, c2b=50, f1w=3600000, f1b=500, f2w=1000, f2b=2)
    reference_names = dict(c1w="conv1_weights.bin", c1b="conv1_biases.bin", c2w="conv2_weights.bin", c2b="conv2_biases.bin",
                           f1w="ip1_weights.bin", f1b="ip1_biases.bin", f2w="ip2_weights.bin", f2b="ip2_biases.bin")
    assert names == sorted(reference_names.values())
    assert sorted(p.name for p in (tmp_path / "params").iterdir()) == names  # and nothing else: no network.cfg
    for k, name in reference_names.items():
        raw = (tmp_path / "params" / name).read_bytes()
        assert len(raw) == 4 * sizes[k], name
        assert raw == np.ascontiguousarray(want[k], "<f4").tobytes(), name
    # the way back, for --init: exact where the scale is a power of two
    back = eigen_export.to_torch(eigen_export.load(str(tmp_path / "params")), scale)
    for k in api.TORCH_KEYS:
        assert back[k].shape == st[k].shape
        if k != "conv1.weight" or scale == 1.0 / 256:
            assert back[k].tobytes() == st[k].tobytes(), k
        else:
            assert np.abs(back[k] - st[k]).max() <= np.spacing(np.abs(st[k]).max())


@pytest.mark.parametrize("scale", [0.0, -1.0 / 256, float("nan"), float("inf")])
def test_export_refuses_a_bad_input_scale(tmp_path, scale):
    with pytest.raises(ValueError, match="input_scale"):
        eigen_export.export(api.init_xavier(3, 1), str(tmp_path / "params"), scale)
    assert not (tmp_path / "params").exists()


def test_export_refuses_a_network_with_conv_relus(tmp_path):
    with pytest.raises(ValueError, match="ReLU"):
        eigen_export.export(api.init_xavier(3, 1), str(tmp_path / "params"), conv_relu=True)
    assert not (tmp_path / "params").exists()


def test_load_fills_what_a_directory_lacks(tmp_path):
    st = api.init_xavier(3, 3)
    eigen_export.export(st, str(tmp_path / "params"))
    (tmp_path / "params" / "ip1_weights.bin").unlink()
    with pytest.raises(FileNotFoundError):
        eigen_export.load(str(tmp_path / "params"))
    fill = api.lenet_from_torch(api.init_xavier(3, 5), 3)
    w = eigen_export.load(str(tmp_path / "params"), fill)
    want = api.lenet_from_torch(st, 3)
    for k in want:
        assert w[k].tobytes() == (fill if k == "f1w" else want)[k].tobytes(), k
