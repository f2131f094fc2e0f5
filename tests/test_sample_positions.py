"""gpd_hip_sample_positions — the draw stream of Cloud::subsample that libgpd_hip.so and the host mirror share
(gpd_amd/csrc/sample_model.h) — against a pure-Python restatement of the stream, and the mirror's Cloud::subsample
against both.  No GPU: the export is host only."""
import numpy as np
import pytest

from gpd_amd import api, hostlib
from pyref_sample import dense_fisher_yates as _dense_fisher_yates, with_repetition as _with_repetition

SEEDS = [0, 1, 7, 12345, 0x9E3779B9, 0xFFFFFFFF]
SIZES = [1, 2, 3, 1000, (1 << 20) + 3]


def _draw_counts(n):
    return sorted({0, 1, max(n - 1, 0), n, n + 5})


def test_the_export_exists():
    assert "gpd_hip_sample_positions" in api.EXPORTS
    getattr(api.lib(), "gpd_hip_sample_positions")


@pytest.mark.parametrize("n", SIZES)
def test_with_repetition_equals_the_restated_stream(n):
    for seed in SEEDS:
        for d in _draw_counts(n):
            got = api.sample_positions(n, d, seed, with_repetition=True)
            want = _with_repetition(n, d, seed)
            assert got.dtype == np.int32 and np.array_equal(got, want), (n, d, seed)
            if d >= n:
                assert np.array_equal(got, np.arange(n)), (n, d, seed)
            assert len(got) == (0 if d == 0 else min(d, n))
            assert got.size == 0 or (got.min() >= 0 and got.max() < n)


@pytest.mark.parametrize("n", SIZES)
def test_without_repetition_equals_the_dense_fisher_yates(n):
    seeds = SEEDS if n <= 1000 else SEEDS[:3]  # a full shuffle of 2^20 entries in pure Python takes a second
    for seed in seeds:
        for d in _draw_counts(n):
            got = api.sample_positions(n, d, seed, with_repetition=False)
            want = _dense_fisher_yates(n, d, seed)
            assert np.array_equal(got, want), (n, d, seed)
            assert len(got) == min(d, n) and len(set(got.tolist())) == len(got), (n, d, seed)
            assert got.size == 0 or (got.min() >= 0 and got.max() < n)


def test_long_draws_from_a_large_list():
    n = (1 << 20) + 3
    for seed in (3, 99):
        got = api.sample_positions(n, 20000, seed, with_repetition=True)
        assert np.array_equal(got, _with_repetition(n, 20000, seed))
        got = api.sample_positions(n, 20000, seed, with_repetition=False)
        assert np.array_equal(got, _dense_fisher_yates(n, 20000, seed))
        assert len(set(got.tolist())) == 20000


def test_seeds_differ_and_repeat():
    a = api.sample_positions(1000, 100, 1, with_repetition=True)
    b = api.sample_positions(1000, 100, 2, with_repetition=True)
    assert not np.array_equal(a, b)
    assert np.array_equal(a, api.sample_positions(1000, 100, 1, with_repetition=True))
    assert len(set(a.tolist())) < 100 or len(set(api.sample_positions(50, 49, 1, with_repetition=True).tolist())) < 49  # it does repeat


def test_bad_arguments_are_refused():
    k = api.C.c_int(-7)
    out = np.zeros(4, np.int32)
    L = api.lib()
    assert L.gpd_hip_sample_positions(-1, 3, 0, 0, api._ptr(out), api.C.byref(k)) == -1
    assert L.gpd_hip_sample_positions(4, 3, 0, 0, api._ptr(out), None) == -1
    assert L.gpd_hip_sample_positions(4, 3, 0, 0, None, api.C.byref(k)) == -1
    assert L.gpd_hip_sample_positions(0, 3, 0, 1, None, api.C.byref(k)) == 0 and k.value == 0
    assert L.gpd_hip_sample_positions(4, -2, 0, 1, api._ptr(out), api.C.byref(k)) == 0 and k.value == 0


@pytest.mark.parametrize("n", [1, 2, 3, 1000, 70001])
def test_the_mirror_draws_the_same(n):
    """util::Cloud::subsample (rewritten on the shared header) gives what it gave: the dense Fisher-Yates without sample
    indices, list[next() % n] draws with them, and leaves the cloud alone for num_samples <= 0."""
    rng = np.random.default_rng(n)
    for seed in SEEDS[:4]:
        for d in _draw_counts(n):
            got = hostlib.subsample_indices(n, d, seed)
            assert np.array_equal(got, _dense_fisher_yates(n, d, seed)), (n, d, seed)
            assert np.array_equal(got, api.sample_positions(n, d, seed, with_repetition=False))
        # a cloud of 3 n points that carries n sample indices
        lst = np.sort(rng.choice(3 * n, n, replace=False)).astype(np.int32)
        for d in _draw_counts(n):
            got = hostlib.subsample_indices(3 * n, d, seed, sample_indices=lst)
            want = lst if d <= 0 else lst[_with_repetition(n, d, seed)]
            assert np.array_equal(got, want), (n, d, seed)
            if d > 0:
                assert np.array_equal(got, lst[api.sample_positions(n, d, seed, with_repetition=True)])
