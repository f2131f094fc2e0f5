"""The host-only entries of the shape-general trainer (gpd_hip_train_net_sizes, _net_init_state, _net_init_xavier):
no GPU is needed."""
import ctypes as C

import numpy as np
import pytest

from gpd_amd import api

SHAPES = [(1, 1, 1, 1, 0), (3, 33, 65, 31, 0), (15, 6, 16, 120, 84), (12, 10, 20, 100, 33), (15, 20, 50, 500, 0), (3, 40, 100, 500, 0)]
BAD = [(2, 20, 50, 500, 0), (3, 0, 50, 500, 0), (3, 65, 50, 500, 0), (3, 20, 129, 500, 0), (3, 20, 50, 0, 0), (3, 20, 50, 1025, 0),
       (3, 20, 50, 500, -1), (3, 20, 50, 500, 1025)]


def _random_state(shape, seed=0):
    rng = np.random.RandomState(seed)
    return {k: rng.rand(*s).astype(np.float32) for k, s in zip(api.net_keys(shape), api.net_state_shapes(shape))}


@pytest.mark.parametrize("dims", SHAPES)
def test_net_sizes_are_torch_net_arrays_shapes(dims):
    shape = api.LenetShape(*dims)
    read, arrs = api.torch_net_arrays(_random_state(shape))
    assert read.as_tuple() == dims
    n = api.net_sizes(shape)
    assert n[:len(arrs)] == [a.size for a in arrs]
    assert n[len(arrs):] == [0] * (10 - len(arrs))
    assert [tuple(a.shape) for a in arrs] == list(api.net_state_shapes(shape))


def _fan_in(dims):
    Cn, F1, F2, H1, H2 = dims
    return [25 * Cn, 25 * F1, 144 * F2, H1, H2]


@pytest.mark.parametrize("dims", SHAPES)
def test_net_init_state_bounds_and_determinism(dims):
    a = api.init_state(dims[0], 7, shape=dims[1:])
    b = api.init_state(dims[0], 7, shape=dims[1:])
    c = api.init_state(dims[0], 8, shape=dims[1:])
    keys = api.net_keys(api.LenetShape(*dims))
    assert tuple(a) == keys and len(keys) == (10 if dims[4] else 8)
    for i, k in enumerate(keys):
        bound = float(np.float32(1.0 / np.sqrt(_fan_in(dims)[i // 2])))
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all()
        assert float(np.abs(a[k]).max()) <= bound, (k, float(np.abs(a[k]).max()), bound)
        assert a[k].tobytes() == b[k].tobytes()
    assert any(a[k].tobytes() != c[k].tobytes() for k in keys)
    # the draws fill the bound: the largest weight tensor comes close to it
    big = max(keys, key=lambda k: a[k].size)
    if a[big].size >= 1000:
        i = keys.index(big)
        assert float(np.abs(a[big]).max()) > 0.95 * float(np.float32(1.0 / np.sqrt(_fan_in(dims)[i // 2])))


@pytest.mark.parametrize("dims", SHAPES)
def test_net_init_xavier_bounds_and_determinism(dims):
    a = api.init_xavier(dims[0], 7, shape=dims[1:])
    b = api.init_xavier(dims[0], 7, shape=dims[1:])
    keys = api.net_keys(api.LenetShape(*dims))
    assert tuple(a) == keys
    for i, k in enumerate(keys):
        if i & 1:
            assert not a[k].any()
        else:
            bound = np.sqrt(3.0 / _fan_in(dims)[i // 2])
            assert float(np.abs(a[k].astype(np.float64)).max()) <= bound, k
        assert a[k].tobytes() == b[k].tobytes()


@pytest.mark.parametrize("channels", [1, 3, 12, 15])
def test_stock_shape_gives_the_bytes_of_the_eight_tensor_functions(channels):
    for seed in (0, 1, 0xFFFFFFFF):
        old, new = api.init_state(channels, seed), api.init_state(channels, seed, shape=(20, 50, 500))
        assert tuple(old) == tuple(new) == api.TORCH_KEYS
        for k in old:
            assert old[k].shape == new[k].shape and old[k].tobytes() == new[k].tobytes(), k
        old, new = api.init_xavier(channels, seed), api.init_xavier(channels, seed, shape=(20, 50, 500, 0))
        for k in old:
            assert old[k].shape == new[k].shape and old[k].tobytes() == new[k].tobytes(), k


def test_a_prefix_of_the_stream():
    """The tensors are drawn in order from one stream: Net and NetCCFFF of the same first three widths share the first six tensors."""
    a, b = api.init_state(3, 5, shape=(6, 16, 120)), api.init_state(3, 5, shape=(6, 16, 120, 84))
    for k in api.TORCH_KEYS[:6]:
        assert a[k].tobytes() == b[k].tobytes()


@pytest.mark.parametrize("dims", BAD)
def test_bad_shapes_are_refused_with_nothing_written(dims):
    L = api.lib()
    shape = api.LenetShape(*dims)
    n = (C.c_size_t * 10)(*([77] * 10))
    assert L.gpd_hip_train_net_sizes(C.byref(shape), n) == -1
    assert list(n) == [77] * 10
    bufs = [np.full(64, 5.0, np.float32) for _ in range(10)]
    ptrs = (C.c_void_p * 10)(*[b.ctypes.data for b in bufs])
    assert L.gpd_hip_train_net_init_state(C.byref(shape), 1, ptrs) == -1
    assert L.gpd_hip_train_net_init_xavier(C.byref(shape), 1, ptrs) == -1
    assert b"limits" in L.gpd_hip_last_error()
    assert all((b == 5.0).all() for b in bufs)
    with pytest.raises(api.GpdHipError):
        api.init_state(dims[0], 1, shape=dims[1:])


def test_null_arguments_are_refused_with_nothing_written():
    L = api.lib()
    shape = api.LenetShape(3, 6, 16, 120, 84)
    assert L.gpd_hip_train_net_sizes(None, (C.c_size_t * 10)()) == -1
    assert L.gpd_hip_train_net_sizes(C.byref(shape), None) == -1
    assert L.gpd_hip_train_net_init_state(C.byref(shape), 1, None) == -1
    arrs, ptrs = api._net_buffers(shape)
    for a in arrs:
        a[...] = 5.0
    ptrs[9] = None  # a NULL among the used slots
    assert L.gpd_hip_train_net_init_state(C.byref(shape), 1, ptrs) == -1
    assert L.gpd_hip_train_net_init_xavier(C.byref(shape), 1, ptrs) == -1
    assert all((a == 5.0).all() for a in arrs)
    # without a third dense layer slots [8] and [9] are not used and may be NULL
    shape8 = api.LenetShape(3, 6, 16, 120, 0)
    arrs, ptrs = api._net_buffers(shape8)
    assert ptrs[8] is None and ptrs[9] is None
    assert L.gpd_hip_train_net_init_state(C.byref(shape8), 1, ptrs) == 0
    assert all(a.any() for a in arrs)


def test_python_shape_arguments():
    assert api.net_shape(3, (6, 16, 120)).as_tuple() == (3, 6, 16, 120, 0)
    assert api.net_shape(15, (6, 16, 120, 84)).as_tuple() == (15, 6, 16, 120, 84)
    with pytest.raises(ValueError):
        api.net_shape(3, (6, 16))
    with pytest.raises(ValueError):
        api.net_shape(3, api.LenetShape(15, 6, 16, 120, 0))
