"""The draws of the importance-sampling driver, host only: gpd_hip_sis_proposals / gpd_hip_sis_select (gpd_amd/csrc/sis_model.h, the
definition the device draw of gpd_hip_detect_sis equals) against the Python restatement tests/pyref_sis.py."""
import ctypes as C

import numpy as np
import pytest

import pyref_sis
from gpd_amd import api

WS_ALL = (-1, 1, -1, 1, -1, 1)


def _cloud(seed=5, n=97):
    rng = np.random.RandomState(seed)
    return rng.uniform(-0.2, 0.2, (n, 3)).astype(np.float32)


def _same(got, want, what):
    assert np.array_equal(got["accepted"], want["accepted"]), what
    assert np.array_equal(got["consumed"], want["consumed"]), what
    assert got["shortfall"] == want["shortfall"], what
    assert got["samples"].tobytes() == want["samples"].tobytes(), what


def _both(centres, g, u, lst, xyz, ws, method, ng, nr, state=(None, None)):
    got = api.sis_select(centres, g, u, lst, xyz, ws, method, ng, nr, state[0])
    want = pyref_sis.select(centres, g, u, lst, xyz, ws, method, ng, nr, state[1])
    return got, want


@pytest.mark.parametrize("seed,rnd,first,count", [(0, 0, 0, 40), (7, 3, 0, 33), (7, 3, 11, 22), (0xFFFFFFF0, 5, 100, 9)])
def test_proposals_equal_the_restatement(seed, rnd, first, count):
    for sigma in (0.02, 0.003):
        got = api.sis_proposals(seed, rnd, 0, first, count, sigma)
        want = pyref_sis.proposals(seed, rnd, 0, first, count, sigma)
        assert np.array_equal(got["idx_raw"], want["idx_raw"])  # exact
        assert got["off"].tobytes() == want["off"].tobytes()    # bit for bit: both sides call this machine's libm
        assert np.all(np.isfinite(got["off"]))
    got = api.sis_proposals(seed, rnd, 1, first, count)
    assert got.dtype == np.uint64 and np.array_equal(got, pyref_sis.proposals(seed, rnd, 1, first, count))
    # a block that starts at `first` is the tail of the block that starts at 0
    whole = api.sis_proposals(seed, rnd, 0, 0, first + count, 0.02)
    assert whole[first:].tobytes() == api.sis_proposals(seed, rnd, 0, first, count, 0.02).tobytes()


def test_streams_are_independent_and_seeded_in_uint32():
    a = api.sis_proposals(1, 0, 1, 0, 8)
    assert not np.array_equal(a, api.sis_proposals(1, 1, 1, 0, 8))
    assert not np.array_equal(a, api.sis_proposals(1, 0, 0, 0, 8)["idx_raw"])
    # round 0's uniform stream of `seed` is the Gaussian stream's seed + 1000003: the same generator from the same state
    assert a[0] == api.sis_proposals(1 + 1000003, 0, 0, 0, 1)["idx_raw"][0]
    assert np.array_equal(api.sis_proposals(2 ** 32 + 9, 2, 1, 0, 5), api.sis_proposals(9, 2, 1, 0, 5))
    assert pyref_sis.stream_seed(0xFFFFFFFF, 3, 1) == (0xFFFFFFFF + 7 * 1000003) % 2 ** 32


def test_proposals_refusals():
    out = np.zeros(4, api.SIS_PROPOSAL_DTYPE)
    f = api.lib().gpd_hip_sis_proposals
    assert f(0, 0, 0, 0, 4, 0.02, api._ptr(out)) == 0
    assert f(0, -1, 0, 0, 4, 0.02, api._ptr(out)) == -1
    assert f(0, 0, 2, 0, 4, 0.02, api._ptr(out)) == -1
    assert f(0, 0, 0, -1, 4, 0.02, api._ptr(out)) == -1
    assert f(0, 0, 0, 0, -1, 0.02, api._ptr(out)) == -1
    assert f(0, 0, 0, 0, 4, 0.0, api._ptr(out)) == -1
    assert f(0, 0, 0, 0, 4, 0.02, None) == -1
    assert f(0, 0, 1, 0, 2, 0.0, api._ptr(out)) == 0  # sigma is not read for the uniform stream
    assert f(0, 0, 0, 0, 0, 0.02, None) == 0


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("L,n_list", [(1, 1), (3, 7), (37, 50), (64, 97)])
def test_select_equals_the_restatement(method, L, n_list):
    xyz = _cloud()
    rng = np.random.RandomState(L * 100 + n_list)
    centres = rng.uniform(-0.1, 0.1, (L, 3))
    lst = rng.randint(0, len(xyz), n_list).astype(np.int32)
    g = api.sis_proposals(11, 2, 0, 0, 400, 0.02)
    u = api.sis_proposals(11, 2, 1, 0, 100)
    ws = (-0.1, 0.15, -0.2, 0.05, -0.15, 0.2)
    inside = np.all((xyz >= np.array(ws[0::2], np.float32)) & (xyz <= np.array(ws[1::2], np.float32)), axis=1)
    if n_list == 1:
        lst = np.flatnonzero(inside)[:1].astype(np.int32)  # a list of one point outside would never fill the round
    got, want = _both(centres, g, u, lst, xyz, ws, method, 28, 12)
    _same(got, want, "L %d, list of %d, method %d" % (L, n_list, method))
    assert got["shortfall"] == 0
    if n_list == 1:
        assert got["consumed"][1] == 12
    else:
        assert not inside[lst].all() and got["consumed"][1] > 12  # the workspace rejected something
    if method == 0 or L == 1:
        assert got["consumed"][0] == 28  # every proposal accepted
    elif L > 3:
        assert got["consumed"][0] > 28   # the nearest-centre test rejected something
    # without a list the uniform source is every point of the cloud
    got, want = _both(centres, g, u, None, xyz, ws, method, 28, 12)
    _same(got, want, "no list")


def test_coincident_centres_tie_is_accepted():
    c = np.array([[0.01, 0.02, 0.03], [0.01, 0.02, 0.03]])
    g = api.sis_proposals(4, 0, 0, 0, 20, 0.02)
    assert set((g["idx_raw"] % 2).tolist()) == {0, 1}
    got, want = _both(c, g, np.zeros(0, np.uint64), None, _cloud(), WS_ALL, 1, 20, 0)
    _same(got, want, "coincident")
    assert got["accepted"][0] == 20 and got["consumed"][0] == 20  # d2 to both is equal: accepted by <=
    assert got["samples"].tobytes() == (c[0] + g["off"]).tobytes()


def test_point_on_a_workspace_bound_is_accepted():
    xyz = np.array([[0.125, 0.0, 0.0], [0.25, 0.0, 0.0], [0.0, -0.5, 0.0], [0.0, 0.0, 0.75], [0.3, 0.0, 0.0]], np.float32)
    u = np.arange(5, dtype=np.uint64)
    ws = (0.0, 0.25, -0.5, 0.0, 0.0, 0.75)  # points 0-3 lie on bounds (all exact in float), point 4 outside
    got, want = _both(np.zeros((1, 3)), np.zeros(0, api.SIS_PROPOSAL_DTYPE), u, None, xyz, ws, 0, 0, 4)
    _same(got, want, "bounds")
    assert got["accepted"][1] == 4 and got["consumed"][1] == 4 and got["shortfall"] == 0
    assert np.array_equal(got["samples"], xyz[:4].astype(np.float64))
    got = api.sis_select(np.zeros((1, 3)), np.zeros(0, api.SIS_PROPOSAL_DTYPE), u[::-1].copy(), None, xyz, ws, 0, 0, 4)
    assert got["consumed"][1] == 5 and np.array_equal(got["samples"], xyz[[3, 2, 1, 0]].astype(np.float64))


def test_a_workspace_that_rejects_everything_reports_the_shortfall():
    xyz = _cloud()
    u = api.sis_proposals(0, 0, 1, 0, 64)
    g = api.sis_proposals(0, 0, 0, 0, 64)
    got, want = _both(np.zeros((2, 3)), g, u, None, xyz, (5, 6, 5, 6, 5, 6), 0, 3, 5)
    _same(got, want, "nothing inside")
    assert got["shortfall"] == 5 and got["accepted"].tolist() == [3, 0] and got["consumed"].tolist() == [3, 64]


@pytest.mark.parametrize("method", [0, 1])
def test_continuation_equals_one_long_block(method):
    xyz = _cloud()
    rng = np.random.RandomState(3)
    centres = rng.uniform(-0.05, 0.05, (23, 3))
    lst = rng.randint(0, len(xyz), 31).astype(np.int32)
    ws = (-0.1, 0.15, -0.2, 0.05, -0.15, 0.2)
    ng, nr = 30, 10
    g = api.sis_proposals(9, 1, 0, 0, 600, 0.02)
    u = api.sis_proposals(9, 1, 1, 0, 300)
    whole = api.sis_select(centres, g, u, lst, xyz, ws, method, ng, nr)
    assert whole["shortfall"] == 0
    st, st_ref, blocks = None, None, 0
    for first in range(0, 600, 7):
        gb, ub = g[first:first + 7], u[first:first + 7]
        st, st_ref = _both(centres, gb, ub, lst, xyz, ws, method, ng, nr, (st, st_ref))
        _same(st, st_ref, "block at %d" % first)
        blocks += 1
        if st["shortfall"] == 0:
            break
        assert st["consumed"][0] == min(first + 7, whole["consumed"][0]) or st["accepted"][0] == ng
    assert blocks > 2
    _same(st, whole, "blocks of 7 against one block")


@pytest.mark.parametrize("prob,ng,nr", [(0.0, 40, 0), (1.0, 0, 40), (0.3, 28, 12), (0.999, 1, 39)])
def test_prob_rand_samples_splits_the_round(prob, ng, nr):
    assert pyref_sis.num_rand_samples(prob, 40) == nr
    xyz = _cloud()
    centres = np.random.RandomState(8).uniform(-0.05, 0.05, (5, 3))
    g = api.sis_proposals(2, 0, 0, 0, 200, 0.02)
    u = api.sis_proposals(2, 0, 1, 0, 200)
    got, want = _both(centres, g, u, None, xyz, WS_ALL, 1, ng, nr)
    _same(got, want, "prob %g" % prob)
    assert got["accepted"].tolist() == [ng, nr] and got["shortfall"] == 0
    if ng == 0:
        assert got["consumed"][0] == 0
        # no Gaussian sample: no centre is needed either
        assert api.sis_select(np.zeros((0, 3)), g[:0], u, None, xyz, WS_ALL, 0, 0, nr)["samples"].tobytes() == got["samples"].tobytes()
    if nr == 0:
        assert got["consumed"][1] == 0


def test_draw_round_restatement_agrees_with_the_library_over_blocks():
    xyz = _cloud()
    centres = np.random.RandomState(1).uniform(-0.05, 0.05, (9, 3))
    want = pyref_sis.draw_round(21, 4, centres, None, xyz, (-0.1, 0.15, -0.2, 0.05, -0.15, 0.2), 1, 40, 0.3, 0.02, block=8)
    g = api.sis_proposals(21, 4, 0, 0, int(want["consumed"][0]), 0.02)
    u = api.sis_proposals(21, 4, 1, 0, int(want["consumed"][1]))
    _same(api.sis_select(centres, g, u, None, xyz, (-0.1, 0.15, -0.2, 0.05, -0.15, 0.2), 1, 28, 12), want, "draw_round")


def test_select_refusals_and_the_job_layout():
    xyz = _cloud()
    g = api.sis_proposals(0, 0, 0, 0, 4)
    with pytest.raises(api.GpdHipError):
        api.sis_select(np.zeros((0, 3)), g, np.zeros(0, np.uint64), None, xyz, WS_ALL, 0, 2, 0)  # Gaussian samples without a centre
    with pytest.raises(api.GpdHipError):
        api.sis_select(np.zeros((1, 3)), g, np.zeros(0, np.uint64), None, xyz, WS_ALL, 2, 2, 0)  # no such method
    with pytest.raises(api.GpdHipError):
        api.sis_select(np.zeros((1, 3)), g, np.ones(3, np.uint64), np.array([len(xyz)], np.int32), xyz, WS_ALL, 0, 2, 1)  # index out of range
    assert api.lib().gpd_hip_sizeof_sis_job() == C.sizeof(api.SisJob) == 192
    assert api.SisJob.workspace.offset == 48 and api.SisJob.hands.offset == 112 and api.SisJob.samples_out.offset == 144
    assert api.SisJob.d2h_bytes.offset == 168 and api.SisJob.stage_ms.offset == 176
    for name in ("gpd_hip_sis_proposals", "gpd_hip_sis_select", "gpd_hip_detect_sis", "gpd_hip_sizeof_sis_job"):
        assert name in api.EXPORTS and hasattr(api.lib(), name)
