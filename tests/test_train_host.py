"""The host-only parts of the trainer (gpd_hip_train_init_state, the refusals that need no device): no GPU."""
import ctypes as C

import numpy as np
import pytest

from gpd_amd import api

FAN_IN = {"conv1": None, "conv2": 500, "fc1": 7200, "fc2": 500}


@pytest.mark.parametrize("channels", [1, 3, 12, 15])
def test_init_state_is_uniform_within_torchs_bounds(channels):
    st = api.init_state(channels, 5)
    assert tuple(st) == api.TORCH_KEYS
    for (k, v), shape in zip(st.items(), api.torch_state_shapes(channels)):
        assert v.shape == shape and v.dtype == np.float32
        fan_in = FAN_IN[k.split(".")[0]] or 25 * channels
        bound = 1.0 / np.sqrt(fan_in)
        assert np.isfinite(v).all() and float(np.abs(v).max()) <= np.float32(bound), k
        # U(-b, b): standard deviation b / sqrt(3); the mean of n draws within 5 standard errors of 0
        assert abs(float(v.astype(np.float64).mean())) <= 5 * bound / np.sqrt(3.0 * v.size), k
        if v.size >= 500:  # ... and it does fill the interval
            assert float(np.abs(v).max()) > 0.98 * bound and abs(float(v.astype(np.float64).std()) / (bound / np.sqrt(3.0)) - 1) < 0.1, k


def test_init_state_is_seeded():
    a, b, c = api.init_state(3, 7), api.init_state(3, 7), api.init_state(3, 8)
    for k in api.TORCH_KEYS:
        assert a[k].tobytes() == b[k].tobytes()
        assert a[k].tobytes() != c[k].tobytes()
    # one stream runs through the eight tensors: no two of them start alike
    assert not np.array_equal(a["conv2.bias"][:20], a["conv1.bias"])


@pytest.mark.parametrize("channels", [2, 0, 16])
def test_init_state_refuses_other_channel_counts(channels):
    L = api.lib()
    arrs = [np.zeros(int(np.prod(s)), np.float32) for s in api.torch_state_shapes(max(channels, 1))]
    ptrs = (C.c_void_p * 8)(*[a.ctypes.data for a in arrs])
    assert L.gpd_hip_train_init_state(channels, 1, ptrs) == -1
    assert b"channels" in L.gpd_hip_last_error()
    with pytest.raises(api.GpdHipError, match="channels"):
        api.init_state(channels, 1)


def test_default_params_are_the_scripts():
    p = api.train_default_params()
    assert (p.channels, p.max_batch) == (15, 64)
    assert (p.lr, p.beta1, p.beta2, p.eps, p.weight_decay, p.input_scale) == (1e-3, 0.9, 0.999, 1e-8, 5e-4, 1.0 / 256)


def test_null_arguments_are_refused_without_a_device():
    L = api.lib()
    out = C.c_void_p()
    assert L.gpd_hip_train_create(None, C.byref(api.train_default_params()), C.byref(out)) == -1
    assert b"gpd_hip_train_create" in L.gpd_hip_last_error()
    assert L.gpd_hip_train_steps(None, None, 1, 1, None) == -1
    assert L.gpd_hip_train_set_state(None, None) == -1
    assert L.gpd_hip_train_kernel_name(0) == b"conv1_forward" and L.gpd_hip_train_kernel_name(99) == b""
