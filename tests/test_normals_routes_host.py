"""The helpers of tests/normals_route_cases.py against the oracle's own neighbour lists, on the CPU: a wrong restatement of the
counts, of the route tally, of the slot demand or of the centroid certificate fails here and not on the device.  And the cases
themselves: every boundary blob yields both B and B + 1 neighbours, the clusters do not see each other, the tiled cloud's
blob lies behind the first tile, the strip's refused points are the tiny point's neighbours."""
from fractions import Fraction

import numpy as np
import pytest

import normals_route_cases as K
import test_centre_certificate as CC


def _oracle_lists(oracle_mod, xyz, radius, rows=None):
    rows = range(len(xyz)) if rows is None else rows
    return {int(i): oracle_mod.radius_search(xyz, xyz[i], radius)[0] for i in rows}


@pytest.fixture(scope="module")
def small():
    return K.small_blobs()


def test_counts_equal_the_oracles_list_lengths(oracle_mod, small):
    deg, strip = K.degenerate_cloud(), K.strip_cloud()
    for xyz, radius in ((small["xyz"], K.RADIUS), (deg["xyz"], K.RADIUS), (strip["xyz"], K.RADIUS), (small["xyz"][:600], 0.012)):
        got = K.counts(xyz, radius)
        mine = K.lists(xyz, radius)
        for i, idx in _oracle_lists(oracle_mod, xyz, radius).items():
            assert got[i] == len(idx)
            assert np.array_equal(mine[i], np.sort(idx))
    # the larger clouds at a sample of their points: the blob, the satellite, the sheet
    for c, rows in ((K.boundary_cloud((4096,), 20 + 4096), [0, 1, 2000, 4095, 4096]), (K.tiled_cloud(), [0, 1, 33000, 65999, 66000, 67099])):
        got = K.counts(c["xyz"], K.RADIUS)
        for i, idx in _oracle_lists(oracle_mod, c["xyz"], K.RADIUS, rows).items():
            assert got[i] == len(idx)


@pytest.mark.parametrize("sizes,seed", [((256, 512, 1024), 11), ((4096,), 20 + 4096), ((8192,), 20 + 8192)])
def test_every_boundary_blob_yields_B_and_B_plus_1(sizes, seed):
    c = K.boundary_cloud(sizes, seed)
    n = K.counts(c["xyz"], K.RADIUS)
    for first, B, sat in c["blobs"]:
        assert len(n[first:first + B]) == B and set(n[first:first + B].tolist()) == {B, B + 1}
        assert n[sat] == 1 + int((n[first:first + B] == B + 1).sum())  # the satellite sees those that see it, and no other cluster
        assert 0.3 * B < n[sat] < 0.6 * B


def test_route_tally_and_slot_demand(oracle_mod, small):
    """from the oracle's list lengths, counted plainly, against tally()"""
    n = np.array([len(v) for _, v in sorted(_oracle_lists(oracle_mod, small["xyz"], K.RADIUS).items())])
    want, demand = K.tally(K.counts(small["xyz"], K.RADIUS))
    queued = [int(v) for v in n if v > 1024]
    assert sorted(set(queued)) == [1025]
    assert want["queued"] == len(queued) and want["queued_lds"] == len(queued) and want["queued_arena"] == 0
    assert demand == 2048 * len(queued)
    # the side of 2^20 this cloud was built for: one attempt on a fresh context, the arena as created
    assert demand < K.ARENA_FRESH and want["attempts"] == 1 and want["arena_slots"] == K.ARENA_FRESH and want["tiles"] == 1
    assert K.register_routes(n) == {4: int((n <= 256).sum()), 8: int(((n > 256) & (n <= 512)).sum()), 16: int(((n > 512) & (n <= 1024)).sum())}
    assert all(v > 0 for v in K.register_routes(n).values())
    assert K.some_wave_is_mixed(want["queued"], len(n))  # queued and small lanes in one wave of the finish kernel
    # hand-made counts at every boundary
    t, d = K.tally([1024, 1025, 4096, 4097, 8192, 8193, 20000])
    assert (t["queued"], t["queued_lds"], t["queued_arena"]) == (6, 4, 2)
    assert d == 2048 + 4096 + 8192 + 8192 + 16384 + 32768 and t["attempts"] == 1
    t, d = K.tally([1025] * 513)
    assert d == 513 * 2048 > K.ARENA_FRESH and t["attempts"] == 2 and t["arena_slots"] == d + d // 8
    t, d = K.tally([1025] * 512)
    assert d == K.ARENA_FRESH and t["attempts"] == 1  # off + m > cap is strict
    t, d = K.tally([2000, 2000, 3000] + [5] * 70000, tile=[0, 0, 1] + [1] * 70000)
    assert t["tiles"] == 2 and d == 4096  # the arena is the next tile's again: the larger of the two
    assert K.pow2ceil([1, 2, 3, 1024, 1025]).tolist() == [1, 2, 4, 1024, 2048]
    assert K.some_wave_is_mixed(70, 200) and not K.some_wave_is_mixed(128, 200) and not K.some_wave_is_mixed(72, 200)


def test_large_blobs_take_both_sort_spaces():
    n = K.counts(K.boundary_cloud((8192,), 20 + 8192)["xyz"], K.RADIUS)
    t, d = K.tally(n)
    assert t["queued"] == 8193 and t["queued_lds"] == int((n <= 8192).sum()) > 0 and t["queued_arena"] == int((n == 8193).sum()) > 0
    assert t["attempts"] == 2 and 0.7e9 < 8 * t["arena_slots"] < 1.0e9
    n = K.counts(K.boundary_cloud((4096,), 20 + 4096)["xyz"], K.RADIUS)
    t, d = K.tally(n)
    assert t["queued"] == t["queued_lds"] == 4097 and t["attempts"] == 2
    assert set(K.pow2ceil(n[:4096]).tolist()) == {4096, 8192}  # one neighbour more doubles the padding


def test_clusters_do_not_see_each_other():
    deg = K.degenerate_cloud()
    n = K.counts(deg["xyz"], K.RADIUS)
    for name, rows in deg["parts"].items():
        assert (n[list(rows)] == len(rows)).all(), name
    assert (deg["cam"][:, list(deg["parts"]["unseen"])] == 0).all() and deg["cam"][:, : deg["parts"]["unseen"][0]].sum(0).min() >= 1
    x = deg["xyz"][list(deg["parts"]["collinear"])].astype(np.float64)
    assert np.array_equal(x[2] - x[1], x[1] - x[0])  # exactly collinear as floats
    assert len(np.unique(deg["xyz"][list(deg["parts"]["identical"])], axis=0)) == 1


def test_tiled_cloud_puts_its_blob_behind_the_first_tile():
    c = K.tiled_cloud()
    n = K.counts(c["xyz"], K.RADIUS)
    assert len(c["xyz"]) > K.TILE + 64 and n[: c["blob"][0]].max() < 256 and (n[list(c["blob"])] == 1100).all()
    assert K.positions_before(c["xyz"], c["blob"]) >= K.TILE
    assert K.grid_of(c["xyz"])[1] == np.float32(0.02)
    tile = np.zeros(len(n), int)
    tile[list(c["blob"])] = 1
    t, d = K.tally(n, tile)
    assert t["tiles"] == 2 and t["queued"] == t["queued_lds"] == 1100 and d == 1100 * 2048 and t["attempts"] == 2


def test_certificate_rule_against_the_entries(oracle_mod, small):
    """centroid_chains against the certificate taken plainly over the oracle's lists (tests/test_centre_certificate.py): where the
    neighbourhood tracks its entries the two are the same rule; where it bounds them by |q| +- rad the bound may only be more
    careful.  And what a certificate promises: the sum is the same in the oracle's order, reversed and exactly."""
    strip = K.strip_cloud()
    rad2 = 2 * np.float32(np.sqrt(np.float32(K.RADIUS * K.RADIUS)) * np.float32(1.0001))
    for xyz in (strip["xyz"], small["xyz"][: 256 + 1]):
        chain, n = K.centroid_chains(xyz, K.RADIUS)
        for i, idx in _oracle_lists(oracle_mod, xyz, K.RADIUS).items():
            assert n[i] == len(idx)
            plain = not all(CC.centre_exact(np.ascontiguousarray(xyz[idx, a])) for a in range(3))
            if (np.abs(xyz[i]) <= rad2).any():
                assert chain[i] == plain, i
            else:
                assert chain[i] or not plain, i
            if not chain[i] and i % 7 == 0:
                for a in range(3):
                    seq = 0.0
                    for v in xyz[idx, a]:
                        seq += float(v)
                    rev = 0.0
                    for v in xyz[idx[::-1], a]:
                        rev += float(v)
                    assert seq == rev and Fraction(seq) == sum(Fraction(float(v)) for v in xyz[idx, a])
    chain, n = K.centroid_chains(strip["xyz"], K.RADIUS)
    near = oracle_mod.radius_search(strip["xyz"], strip["xyz"][strip["tiny"]], K.RADIUS)[0]
    assert np.array_equal(np.flatnonzero(chain), np.sort(near))  # refused: exactly the neighbours of the tiny point
    assert 0 < chain.sum() < len(chain) and n.max() <= K.NL_CAP and K.some_wave_is_mixed(int(chain.sum()), len(chain))
    assert (np.abs(strip["xyz"][:, 0]) <= rad2).all()  # every neighbourhood of the strip tracks its entries
    chain, _ = K.centroid_chains(small["xyz"], K.RADIUS)
    assert not chain.any()  # decimetres from every coordinate plane: certified from |q| +- rad alone
    assert K.centre_exact([255, 110, 109, 100], [0, 126, 126, 255], [5, 4096, 4096, 2]).tolist() == [True, True, False, False]


def test_grid_restatement():
    from gpd_amd import synth
    xyz = synth.make_cloud(77, 3000)["xyz"]
    assert K.grid_of(xyz)[1] == np.float32(0.02)
    assert K.grid_of(K.with_far_pair(xyz, 6.0))[1] == np.float32(0.04)
    assert K.grid_of(K.with_far_pair(xyz, 30.0))[1] == np.float32(0.16)
    assert K.grid_of(K.flat_cloud())[2][2] == 1 and K.grid_of(xyz[:1])[2].tolist() == [1, 1, 1]
    for gap in (6.0, 30.0):  # the far points see nobody, and nobody sees them
        n = K.counts(K.with_far_pair(xyz, gap), K.RADIUS)
        assert n[-2:].tolist() == [1, 1] and np.array_equal(n[:-2], K.counts(xyz, K.RADIUS))
    col7, col10 = K.cell_columns(xyz, 0.07), K.cell_columns(xyz, 0.1)
    assert 0 < (col7 > 64).sum() < len(xyz)          # radius 0.07: both visits in one launch
    assert (col7 > 64).sum() < (col10 > 64).sum() < len(xyz)  # radius 0.1: more of them (the border of so small a grid clamps the rest)
    assert (K.cell_columns(xyz, 0.03) <= 64).all()


def test_eigh_form_on_a_plane():
    rng = np.random.RandomState(3)
    xyz = np.stack([rng.uniform(0, 0.05, 400), rng.uniform(0, 0.05, 400), np.full(400, 0.5)], 1).astype(np.float32)
    nrm, gap = K.eigh_normals(xyz, K.RADIUS)
    assert np.abs(np.abs(nrm[:, 2]) - 1).max() < 1e-12 and gap.min() > 0.05
