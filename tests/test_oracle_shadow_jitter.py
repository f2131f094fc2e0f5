"""The oracle's statement of the seeded shadow jitter (gpd_oracle_set_shadow_jitter, written in oracle/gpd_oracle.cpp from the
definition in include/gpd_hip.h), no GPU: its draw against the numpy statement (tests/pyref_jitter.py) and the library's host
model (gpd_amd/csrc/jitter_model.h) bit for bit; its images against the per-point numpy restatement byte for byte; and the
properties every expectation of tests/entry_cases.py rests on — only the shadow channels move, the candidates and the stream of
shadow draws do not, the seed matters, without a shadow channel nothing changes, and off is off again afterwards."""
import numpy as np
import pytest

import entry_cases as ec
import pyref
import pyref_jitter as J
from gpd_amd import api

SEED = ec.JITTER_SEED
SEEDS = (0, 1, 0x5EED5EED5EED, 2 ** 64 - 1)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
SHADOW = [4, 9, 14]
OTHERS = [c for c in range(15) if c not in SHADOW]


# ---- the draw ---------------------------------------------------------------------------------------------------------------
def _voxels():
    rng = np.random.RandomState(11)
    edge = [I32_MIN, I32_MIN + 1, -65536, -3, -1, 0, 1, 65535, I32_MAX - 1, I32_MAX]
    grid = np.array([(x, y, z) for x in edge for y in edge for z in edge], np.int64)
    base = np.array([[17, -23, 5]], np.int64)
    one_axis = np.concatenate([base + d * np.eye(3, dtype=np.int64)[a][None] for a in range(3) for d in (-1, 1, 1 << 16, -(1 << 20))])
    near = rng.randint(-400, 400, (3000, 3))
    wide = rng.randint(I32_MIN, I32_MAX, (3000, 3), dtype=np.int64)
    return np.concatenate([grid, base, one_axis, near, wide]).astype(np.int32), len(grid), 1 + len(one_axis)


@pytest.mark.parametrize("seed", SEEDS)
def test_draws_of_oracle_numpy_and_library_agree(oracle_mod, seed):
    v, n_grid, n_axis = _voxels()
    assert (v < 0).any() and (v == I32_MIN).any() and (v == I32_MAX).any() and (v == 0).all(axis=1).any()
    got = oracle_mod.shadow_jitter_draws(seed, v)
    assert got.dtype == np.float64 and got.shape == (len(v),)
    assert got.tobytes() == J.draws(seed, v).tobytes()
    assert got.tobytes() == api.shadow_jitter_model(seed, v).tobytes()
    # voxels that differ in one coordinate only draw differently: x, y and z all enter
    one = got[n_grid:n_grid + n_axis]
    assert len(set(one.tolist())) == len(one), one


def test_draws_depend_on_the_whole_seed(oracle_mod):
    v = _voxels()[0][:200]
    a = oracle_mod.shadow_jitter_draws(SEED, v)
    assert a.tobytes() != oracle_mod.shadow_jitter_draws(SEED & 0xFFFFFFFF, v).tobytes()  # above 2^32
    assert a.tobytes() != oracle_mod.shadow_jitter_draws(SEED ^ 1, v).tobytes()


# ---- images against the per-point restatement ------------------------------------------------------------------------------
def _radius(p):
    return max(p.volume_depth, p.volume_height / 2.0, p.volume_width)


def _restate(p, cl, hands, num_sets, seed):
    """The images of every candidate of the first `num_sets` live sets of `hands` at lcg_base 0, in candidate order, and over
    them the count of voxels in a box only because they were moved and out of one only because they were moved."""
    rng = pyref.Lcg(0)
    cam, vp = cl["cam_source"], cl["view_points"]
    want, stats, done = [], dict(moved_in=0, moved_out=0, in_box=0), 0
    for s in range(hands.shape[0]):
        if not hands[s]["valid"].any():
            continue
        if done == num_sets:
            break
        nbr = pyref.radius_neighbours(cl["xyz"], hands[s, 0]["sample"].astype(np.float32), _radius(p))
        if cam.shape[0] == 1:
            vox = J.shadow_voxels(cl["xyz"][nbr], vp[0], rng, _radius(p))
        else:
            vox = J.shadow_voxels_cameras(cl["xyz"][nbr], cam[:, nbr], vp, rng, _radius(p))
        va = np.asarray(vox, np.int64).reshape(-1, 3)
        for h in hands[s][hands[s]["valid"].astype(bool)]:
            want.append(J.grasp_image_jitter(p, h, cl["xyz"], cl["normals"], nbr, vox, seed))
            a, b = J.in_box(p, h, J.lattice_points(va)), J.in_box(p, h, J.shadow_points(va, seed))
            stats["moved_in"] += int((b & ~a).sum())
            stats["moved_out"] += int((a & ~b).sum())
            stats["in_box"] += int(b.sum())
        done += 1
    assert done == num_sets
    return np.stack(want), stats


@pytest.mark.parametrize("name,num_sets", [("default_c15", 2), ("two_cameras", 1)])
def test_images_equal_the_numpy_restatement(oracle_mod, name, num_sets):
    om = oracle_mod
    p, cl, _, _ = ec.inputs(name, om.default_params)
    hands = ec.given_sets(om, name)["a"]
    live = np.flatnonzero(hands["valid"].astype(bool).any(axis=1))[:num_sets]
    head = np.ascontiguousarray(hands[: live[-1] + 1])  # the compared sets and the dead ones before them: the stream starts at 0
    want, stats = _restate(p, cl, head, num_sets, SEED)
    print(name, stats, "over", len(want), "candidates")
    assert stats["moved_in"] >= 1 and stats["moved_out"] >= 1, stats
    with om.shadow_jitter(SEED):
        img, cand = om.images(p, cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"], head)
    assert len(img) == len(want) >= num_sets
    for k in range(len(want)):
        bad = [c for c in range(15) if not np.array_equal(img[k][..., c], want[k][..., c])]
        assert not bad, (name, "candidate %d: channels %s differ, %d pixels" % (k, bad, int((img[k] != want[k]).sum())))
    assert all((im[..., SHADOW] > 0).any() for im in img)
    off, _ = om.images(p, cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"], head)
    assert off[..., SHADOW].tobytes() != want[..., SHADOW].tobytes()  # the restatement with the points on the lattice is another image


# ---- properties on the variants every entry runs on --------------------------------------------------------------------------
def _images(om, name, sets):
    p, cl, _, _ = ec.inputs(name, om.default_params)
    img, cand = om.images(p, cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"], sets)
    return img, cand, om.last_lcg_draws()


@pytest.mark.parametrize("name", ec.JITTER_VARIANTS)
def test_only_the_shadow_channels_move_and_off_is_off_again(oracle_mod, name):
    om = oracle_mod
    sets = ec.given_sets(om, name)["a"]
    C = ec.inputs(name, om.default_params)[0].image_num_channels
    assert om.shadow_jitter_state() is None
    off, cand0, d0 = _images(om, name, sets)
    with om.shadow_jitter(SEED):
        assert om.shadow_jitter_state() == SEED
        on, cand1, d1 = _images(om, name, sets)
    with om.shadow_jitter(SEED + 1):
        on2, cand2, d2 = _images(om, name, sets)
    assert om.shadow_jitter_state() is None
    back, cand3, d3 = _images(om, name, sets)
    assert len(cand0) > 0 and np.array_equal(cand0, cand1) and np.array_equal(cand0, cand2) and np.array_equal(cand0, cand3)
    assert d0 == d1 == d2 == d3
    assert back.tobytes() == off.tobytes()
    if C != 15:
        assert name == "default_c12" and d0 == 0
        assert on.tobytes() == off.tobytes() == on2.tobytes()
        return
    assert d0 > 0
    assert on[..., OTHERS].tobytes() == off[..., OTHERS].tobytes() == on2[..., OTHERS].tobytes()
    for c in SHADOW:
        assert on[..., c].tobytes() != off[..., c].tobytes() and on[..., c].tobytes() != on2[..., c].tobytes(), c
    changed = (on != off).reshape(len(on), -1).any(axis=1)
    assert changed.sum() >= 0.9 * len(on), (int(changed.sum()), len(on))  # the setting reaches (nearly) every candidate's image


def test_the_context_manager_switches_off_when_the_body_raises_and_does_not_nest(oracle_mod):
    om = oracle_mod
    with pytest.raises(KeyError):
        with om.shadow_jitter(SEED):
            raise KeyError("body")
    assert om.shadow_jitter_state() is None
    with om.shadow_jitter(SEED):
        with pytest.raises(RuntimeError):
            with om.shadow_jitter(SEED + 1):
                pass
        assert om.shadow_jitter_state() == SEED
    assert om.shadow_jitter_state() is None
    with om.shadow_jitter(None):
        assert om.shadow_jitter_state() is None


def test_the_expectation_cache_keeps_the_settings_apart(oracle_mod):
    om = oracle_mod
    name = "default_c15"
    off = ec.given(om, name, "a", 0)
    with ec.jitter(om, SEED):
        on = ec.given(om, name, "a", 0)
        assert ec.given(om, name, "a", 0) is on
    with ec.jitter(om, SEED + 1):
        on2 = ec.given(om, name, "a", 0)
    assert ec.given(om, name, "a", 0) is off and on is not off and on2 is not on
    assert on["images"].tobytes() != off["images"].tobytes() and on2["images"].tobytes() != on["images"].tobytes()
    assert on["scores"].tobytes() != off["scores"].tobytes()
    assert on["draws"] == off["draws"] and np.array_equal(on["cand"], off["cand"])
