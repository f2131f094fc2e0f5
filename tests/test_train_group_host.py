"""The definition of training on several replicas (gpd_amd/csrc/group_model.h), host only: the fixed-order mean, the
slices, and the schedule gpd_hip_train_group_steps enqueues — executed here by a small interpreter on numpy arrays under random
interleavings of the streams, with HIP's rule for a wait (it binds to the record of its event that was ENQUEUED last; with none
it passes at once)."""
import numpy as np
import pytest

from gpd_amd import api

F32_MAX = np.finfo(np.float32).max
SIZES = [500 * C + 3626572 for C in (1, 3, 12, 15)] + [1, 3, 4, 5, 17]


def _inputs(G, seed):
    rng = np.random.RandomState(seed)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-39, 1e-12, 0.05, -0.05, F32_MAX, -F32_MAX, F32_MAX / 2, 1.0, -1.0,
                        2.0 ** -126, 3.0, 1e30, -1e30], np.float32)
    g = []
    for r in range(G):
        a = (rng.randn(4099) * 10.0 ** rng.uniform(-12, 2, 4099)).astype(np.float32)
        # every pair of special values meets in some element of replicas 0 and 1, and again deeper in the chain
        grid = np.stack(np.meshgrid(special, special, indexing="ij"), -1).reshape(-1, 2)
        a[:len(grid)] = grid[:, r % 2] if r < 2 else special[rng.randint(0, len(special), len(grid))]
        g.append(a)
    # 1e-12 beside 0.05, in both orders
    g[0][400:402] = [0.05, 1e-12]
    if G > 1:
        g[1][400:402] = [1e-12, 0.05]
    return g


@pytest.mark.parametrize("G", [1, 2, 3, 4, 5])
def test_mean_is_the_numpy_float32_expression(G):
    g = _inputs(G, 40 + G)
    with np.errstate(over="ignore", invalid="ignore"):
        s = g[0].copy()
        for r in range(1, G):
            s = s + g[r]
        want = s * np.float32(1.0 / G)
    assert want.dtype == np.float32
    got = api.train_group_mean(g)
    assert got.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all()  # inf - inf behind an overflow: a NaN on both sides, whatever its payload
    assert got.view(np.uint32)[~nan].tobytes() == want.view(np.uint32)[~nan].tobytes()
    if G == 1:
        assert got.tobytes() == g[0].tobytes()
        assert np.signbit(got[18]) and got[18] == 0  # element 18 pairs special[1] = -0 with special[0]: -0 stays -0
    else:
        assert np.isinf(want).any() and (want == 0).any() and (np.abs(want[want != 0]) < 2.0 ** -126).any()


def test_mean_keeps_the_shape_and_refuses_nonsense():
    a = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    assert api.train_group_mean([a, a]).shape == (2, 3, 4)
    with pytest.raises(ValueError):
        api.train_group_mean([])
    with pytest.raises(ValueError):
        api.train_group_mean([a, a[:1]])
    with pytest.raises(api.GpdHipError, match="17 gradients"):
        api.train_group_mean([a] * 17)


@pytest.mark.parametrize("G", range(1, 17))
def test_slices(G):
    for n in SIZES:
        first = api.train_group_slices(n, G)
        assert first.shape == (G + 1,) and first[0] == 0 and first[-1] == n
        sizes = np.diff(first)
        assert (sizes >= 0).all()  # contiguous, in order: [0, n) exactly once
        assert (first[:-1] % 4 == 0).all()
        assert sizes.max() - sizes.min() <= 4, (n, G, sizes)
    with pytest.raises(api.GpdHipError):
        api.train_group_slices(10, 0)
    with pytest.raises(api.GpdHipError):
        api.train_group_slices(10, 17)


def test_the_uneven_buffer():
    """C = 3: 907 018 quads over 3 owners"""
    first = api.train_group_slices(3628072, 3)
    assert 3628072 == 4 * 907018 and sorted(np.diff(first).tolist()) == [4 * 302339, 4 * 302339, 4 * 302340]


# ---- the schedule, simulated ------------------------------------------------------------------------------------------------

N = 37  # floats of the simulated buffer: the slices of every G <= 4 differ, the last quad is short


def _statics(G, ops):
    """List-order facts: every wait has a record of its event ahead of it; -> for each op index of a wait, the index of the
    record it binds to"""
    last, binds = {}, {}
    for i, op in enumerate(ops):
        if op["kind"] == api.OP_RECORD:
            last[int(op["event"])] = i
        elif op["kind"] == api.OP_WAIT:
            assert int(op["event"]) in last, "op %d waits on event %d, which no earlier op records" % (i, op["event"])
            binds[i] = last[int(op["event"])]
    return binds


def _simulate(G, steps, ops, binds, rng, grads):
    """Runs the list under one random interleaving -> per (replica, step), the replica's gradient buffer as its update saw it"""
    first = api.train_group_slices(N, G)
    weight = np.float32(1.0 / G)
    d_g = [np.full(N, np.nan, np.float32) for _ in range(G)]
    gather = [np.full((max(G - 1, 1), N), np.nan, np.float32) for _ in range(G)]
    queues = [[i for i, op in enumerate(ops) if op["stream"] == r] for r in range(G)]
    head, done = [0] * G, set()
    step, seen = [0] * G, {}
    row = lambda o, r: r if r < o else r - 1
    while any(head[r] < len(queues[r]) for r in range(G)):
        ready = [r for r in range(G) if head[r] < len(queues[r])
                 and not (ops[queues[r][head[r]]]["kind"] == api.OP_WAIT and binds[queues[r][head[r]]] not in done)]
        assert ready, "deadlock: every stream's head waits on a record that cannot run"
        r = ready[rng.randint(len(ready))]
        i = queues[r][head[r]]
        op = ops[i]
        kind, peer, sl = int(op["kind"]), int(op["peer"]), int(op["slice"])
        if kind == api.OP_BACKWARD:
            d_g[r][:] = grads[r][step[r]]
        elif kind == api.OP_COPY:
            a, b = first[sl], first[sl + 1]
            if sl == r:
                gather[r][row(r, peer), :b - a] = d_g[peer][a:b]
            else:
                d_g[r][a:b] = d_g[peer][a:b]
        elif kind == api.OP_SUM:
            assert sl == r
            a, b = first[sl], first[sl + 1]
            s = None
            for q in range(G):
                v = d_g[r][a:b] if q == r else gather[r][row(r, q), :b - a]
                s = v.copy() if s is None else s + v
            d_g[r][a:b] = s * weight
            gather[r][:] = np.nan  # a row read again without being refilled shows
        elif kind == api.OP_UPDATE:
            seen[(r, step[r] - 1)] = d_g[r].copy()
        done.add(i)
        head[r] += 1
        if kind == api.OP_BACKWARD:
            step[r] += 1
    assert step == [steps] * G
    return seen


@pytest.mark.parametrize("G", [1, 2, 3, 4])
def test_schedule_under_random_interleavings(G):
    steps = 2
    ops = api.train_group_schedule(G, steps)
    assert ops.dtype == api.GROUP_OP_DTYPE and ops.dtype.itemsize == 20
    assert set(ops["kind"].tolist()) <= set(range(6)) and ((ops["stream"] >= 0) & (ops["stream"] < G)).all()
    for r in range(G):
        mine = ops[ops["stream"] == r]
        assert (mine["kind"] == api.OP_BACKWARD).sum() == steps and (mine["kind"] == api.OP_UPDATE).sum() == steps
    # an event is recorded on one stream only (it lives on that replica's device)
    rec = ops[ops["kind"] == api.OP_RECORD]
    assert all(len(set(rec["stream"][rec["event"] == e].tolist())) == 1 for e in set(rec["event"].tolist()))
    binds = _statics(G, ops)
    rng = np.random.RandomState(700 + G)
    grads = [[(rng.randn(N) * 10.0 ** rng.uniform(-6, 1, N)).astype(np.float32) for _ in range(steps)] for _ in range(G)]
    want = [api.train_group_mean([grads[r][s] for r in range(G)]) for s in range(steps)]
    for trial in range(250):
        seen = _simulate(G, steps, ops, binds, np.random.RandomState(1000 * G + trial), grads)
        for r in range(G):
            for s in range(steps):
                assert seen[(r, s)].tobytes() == want[s].tobytes(), (G, trial, r, s)


def test_the_simulation_catches_a_missing_wait():
    """The interpreter is worth its name only if a schedule with a hole fails under it: drop, in turn, one wait of each phase."""
    G, steps = 3, 2
    ops = api.train_group_schedule(G, steps)
    rng = np.random.RandomState(5)
    grads = [[(rng.randn(N)).astype(np.float32) for _ in range(steps)] for _ in range(G)]
    want = [api.train_group_mean([grads[r][s] for r in range(G)]) for s in range(steps)]
    waits = [i for i, op in enumerate(ops) if op["kind"] == api.OP_WAIT]
    for phase in range(3):  # events of the gradients, the sums, the gathered buffers
        drop = next(i for i in waits if int(ops[i]["event"]) // G == phase)
        cut = np.delete(ops, drop)
        binds = _statics(G, cut)
        wrong = 0
        for trial in range(250):
            seen = _simulate(G, steps, cut, binds, np.random.RandomState(trial), grads)
            wrong += any(seen[(r, s)].tobytes() != want[s].tobytes() for r in range(G) for s in range(steps))
        assert wrong > 0, "dropping wait %d (event %d) went unnoticed" % (drop, ops[drop]["event"])


def test_schedule_sizes_and_refusals():
    assert len(api.train_group_schedule(3, 0)) == 0
    one, two = api.train_group_schedule(3, 1), api.train_group_schedule(3, 2)
    assert two[:len(one)].tobytes() == one.tobytes()  # a prefix: the first step does not know what follows
    assert len(two) == 2 * len(one) + 3 * 2            # the second step's waits on the gathered buffers
    assert [int(k) for k in api.train_group_schedule(1, 2)["kind"]] == [api.OP_BACKWARD, api.OP_UPDATE] * 2
    k = api.C.c_int(0)
    buf = np.zeros(4, api.GROUP_OP_DTYPE)
    assert api.lib().gpd_hip_train_group_schedule(3, 1, buf.ctypes.data_as(api.C.c_void_p), 4, api.C.byref(k)) == -3
    assert k.value == len(one)
    with pytest.raises(api.GpdHipError):
        api.train_group_schedule(0, 1)
    with pytest.raises(api.GpdHipError):
        api.train_group_schedule(17, 1)
    for name in ("gpd_hip_train_group_mean", "gpd_hip_train_group_slices", "gpd_hip_train_group_schedule", "gpd_hip_train_group_create",
                 "gpd_hip_train_group_destroy", "gpd_hip_train_group_broadcast", "gpd_hip_train_group_steps", "gpd_hip_train_group_verify",
                 "gpd_hip_train_group_last_bytes"):
        assert name in api.EXPORTS and getattr(api.lib(), name)
