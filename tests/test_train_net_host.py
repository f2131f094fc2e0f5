"""The host-only entries of the shape-general trainer (gpd_hip_train_net_sizes, _net_init_state, _net_init_xavier):
no GPU is needed.  Further down, the conditions that test_gpu_train_net_edges.py's inputs stand for, on the float64 references."""
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


# ---- the conditions of test_gpu_train_net_edges.py that need no device (float64 on the CPU) -------------------------------------

def test_the_general_sgd_reference_is_the_stock_one_at_the_stock_shape():
    """train_net_ref.sgd_trajectory and train_caffe_ref.sgd_trajectory share the rule (caffe_sgd_trajectory); at the stock
    widths, where both can run, they give the same bytes, multipliers included."""
    import torch
    import train_caffe_ref as cr
    import train_net_ref as nr
    from test_gpu_train_caffe import N_SET, ROWS
    st, img, lab = cr.xavier_state(3), cr.images(3)[:N_SET], cr.labels()[:N_SET]
    lm, dm = {"conv2.weight": 0.0, "fc1.bias": 2.0}, {"fc2.bias": 0.0}
    for dtype in (torch.float64, torch.float32):
        la, sa = cr.sgd_trajectory(st, img, lab, ROWS[:2], dtype, None, lm, dm)
        lb, sb = nr.sgd_trajectory(st, img, lab, ROWS[:2], dtype, None, lm, dm, conv_relu=False)
        assert la.tobytes() == lb.tobytes() and tuple(sa) == tuple(sb) == api.TORCH_KEYS
        assert all(sa[k].tobytes() == sb[k].tobytes() for k in sa)
    assert sa["conv2.weight"].tobytes() == st["conv2.weight"].tobytes()


def test_the_sgd_cases_move_what_they_should_and_differ():
    """Every SGD case's float64 reference moves every unfrozen tensor by more than 1e-5 (fc3.* among them: their update is
    observed), and the references of the cases differ from one another by far more than their allowances: a device that
    ignored the policy, a multiplier or the tensor a slot belongs to could not pass them all."""
    import torch
    import train_net_ref as nr
    out = {}
    for case in nr.SGD_CASES:
        widths, st0, img, lab, rows, hyper, lm, dm = nr.sgd_case(case)
        l64, s64, el32, e32 = nr.sgd_trajectory_yardstick(st0, img, lab, rows, hyper, lm, dm)
        moved = nr.check_sgd_moves(case, st0, s64, lm)
        print(case, {k: "%.3g" % m for k, m in moved.items()})
        out[case] = (s64, e32)
    for a, b, k in (("ccfff inv", "ccfff step", "fc3.weight"), ("ccfff inv", "ccfff step", "fc1.weight"),
                    ("frozen", "no bias decay", "conv1.weight"), ("frozen", "no bias decay", "fc1.bias"), ("frozen", "no bias decay", "conv2.bias")):
        diff = float(np.abs(out[a][0][k] - out[b][0][k]).max())
        allow = nr.FACTOR * max(out[a][1][k], out[b][1][k])
        print("%s against %s, %s: %.3g apart, allowance %.3g" % (a, b, k, diff, allow))
        assert diff > 10 * allow and diff > 1e-7
    # the decay multiplier alone: the biases of (7, 9, 33) with and without decay, nothing frozen
    widths, st0, img, lab, rows, hyper, lm, dm = nr.sgd_case("no bias decay")
    plain = nr.sgd_trajectory(st0, img, lab, rows, torch.float64, hyper)[1]
    for k in nr.SGD_BIASES:
        diff = float(np.abs(plain[k] - out["no bias decay"][0][k]).max())
        print("decay_mult 0 on %s: %.3g apart, allowance %.3g" % (k, diff, nr.FACTOR * out["no bias decay"][1][k]))
        assert diff > nr.FACTOR * out["no bias decay"][1][k] and diff > 1e-7


@pytest.mark.parametrize("B", [7, 9, 33, 257])
def test_the_batch_edges_reach_every_tensor(B):
    import torch
    import train_net_ref as nr
    import train_ref as tr
    dims = nr.BATCH_DIMS
    idx = nr.batch_indices(B, 257)
    for caffe in ((False, True) if B == 33 else (False,)):
        g64, _ = nr.autograd(api.init_state(dims[0], nr.BATCH_SEED, shape=dims[1:]), tr.images(1, n=257)[idx], tr.labels(257)[idx], torch.float64, conv_relu=not caffe)
        assert all(np.abs(g).max() > 0 for g in g64.values())
    assert set(tr.labels(257)[idx].tolist()) == {0, 1}


def test_which_term_sizes_the_partial_buffer():
    """16 H1 decides at train_net_ref.PART_DIMS, 80 times the next term at the least; it also does, by less (528 against 375,
    8000 against 2400), at the narrow one-channel shapes of the batch edges and the head probes and at H1 = 500 behind narrow
    convolutions.  At every other shape the suite trains, a convolution's partials decide."""
    import train_net_ref as nr
    for dims in nr.PART_DIMS:
        a, b, c = nr.part_terms(dims)
        assert c >= 80 * max(a, b), (dims, a, b, c)
    for dims in (nr.BATCH_DIMS, (1, 3, 5, 33, 84), (1, 3, 5, 33, 500), (3, 6, 16, 500, 0), (3, 6, 16, 500, 84)):
        a, b, c = nr.part_terms(dims)
        assert c > max(a, b), (dims, a, b, c)
    for dims in SHAPES + [(1, 64, 128, 1024, 1024), (3, 6, 16, 120, 84), (3, 7, 9, 33, 0), (3, 6, 16, 120, 500)]:
        a, b, c = nr.part_terms(dims)
        assert c <= max(a, b), (dims, a, b, c)


@pytest.mark.parametrize("dims,seed", [((1, 1, 1, 1024, 0), 2), ((1, 2, 3, 1000, 7), 2), ((3, 6, 16, 120, 500), 2), ((3, 6, 16, 500, 0), 2), ((3, 6, 16, 500, 84), 2)])
def test_the_wide_shapes_reach_every_tensor(dims, seed):
    import torch
    import train_net_ref as nr
    import train_ref as tr
    idx = nr.batch_indices(5, 70)
    g64, _ = nr.autograd(api.init_state(dims[0], seed, shape=dims[1:]), tr.images(dims[0])[idx], tr.labels()[idx], torch.float64)
    assert all(np.abs(g).max() > 0 for g in g64.values()), {k: float(np.abs(g).max()) for k, g in g64.items()}


@pytest.mark.parametrize("layer,live", [("fc2", None), ("fc2", 37), ("fc1", None), ("fc1", 53)])
def test_dead_layers_in_float64(layer, live):
    import torch
    import train_net_ref as nr
    import train_ref as tr
    Cn = nr.DEAD_DIMS[0]
    st = nr.dead_state(layer, live)
    g64, l64 = nr.autograd(st, tr.images(Cn)[nr.DEAD_IDX], tr.labels()[nr.DEAD_IDX], torch.float64)
    nr.check_dead_reference(layer, live, g64)
    assert set(tr.labels()[nr.DEAD_IDX].tolist()) == {0, 1} and np.isfinite(l64)


def test_head_margins_in_float64():
    import train_net_ref as nr
    st, d = nr.both_branches_state()
    print("both branches:", np.array2string(np.sort(d), precision=3))
    st, d = nr.saturated_state()
    print("saturated:", np.array2string(np.sort(d), precision=1))
    st, z64, e32 = nr.eval_state()
    print("eval: smallest |margin| %.3g, e32 %.3g" % (float(np.abs(z64[:, 1] - z64[:, 0]).min()), e32))
