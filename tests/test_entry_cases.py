"""The expectations of tests/entry_cases.py are not empty: with the oracle alone, every variant of tests/ref_cases.py gives every
composed entry something to be wrong about.  The counts below are the oracle's own (8000 points, 24 samples per variant); the
conditions that tests/test_gpu_entries_by_variant.py rests on are asserted from them."""
import numpy as np
import pytest

import entry_cases as ec
import ref_cases as rcs

# variant -> (detect candidates, detect_sis live sets per pass, detect_sis hands, label_view (candidates, positives, kept))
DEFAULT = (51, [17, 13, 10], 122, (128, 3, 6))
OFFLATTICE = (42, [16, 8, 13], 106, (128, 3, 6))
COUNTS = {
    "axis1_four_orientations": (13, [8, 4, 8], 34, (40, 1, 2)),
    "deep_hand": (58, [17, 14, 8], 132, (145, 4, 8)),
    "default_c1": DEFAULT,
    "default_c12": DEFAULT,
    "default_c15": DEFAULT,
    "default_c3": DEFAULT,
    "frame_radius": (43, [16, 13, 14], 120, (134, 1, 2)),
    "friction_viable_aperture": (19, [12, 7, 9], 51, (52, 2, 4)),
    "huge_image_volume": DEFAULT,
    "no_deepen": (55, [17, 13, 11], 133, (146, 0, 0)),
    "offlattice_c15": OFFLATTICE,
    "offlattice_c3": OFFLATTICE,
    "offlattice_three_axes": (103, [19, 11, 11], 249, (334, 6, 12)),
    "offlattice_two_cameras": OFFLATTICE,
    "other_image_volume": DEFAULT,
    "six_placements_wide_fingers": (45, [17, 13, 10], 112, (118, 2, 4)),
    "small_hand": (51, [17, 9, 10], 111, (112, 0, 0)),
    "three_axes": (108, [19, 11, 10], 242, (341, 6, 12)),
    "three_cameras": DEFAULT,
    "tight_workspace": (5, [3, 4, 4], 22, (15, 0, 0)),
    "twelve_cameras": DEFAULT,
    "twelve_orientations": (75, [17, 13, 11], 180, (194, 5, 10)),
    "two_cameras": DEFAULT,
    "wide_image_volume": DEFAULT,
}
# no positive among the view's candidates: there the label_view comparison rests on all_labels, round_counts and the empty output
VIEW_KEEPS_NOTHING = ("no_deepen", "small_hand", "tight_workspace")
FEW_IMAGES = ("tight_workspace",)  # five candidates: no share of non-empty images is asked of it


def test_the_table_names_every_variant():
    assert sorted(COUNTS) == sorted(rcs.VARIANTS) and len(COUNTS) == 24
    assert all(n in COUNTS for n in VIEW_KEEPS_NOTHING + FEW_IMAGES)


@pytest.mark.parametrize("name", sorted(rcs.VARIANTS))
def test_no_expectation_is_empty(oracle_mod, name):
    _proofs(oracle_mod, name)


@pytest.mark.parametrize("name", ec.JITTER_VARIANTS)
def test_no_expectation_is_empty_with_the_shadow_jitter_on(oracle_mod, name):
    """The same proofs on the expectations of gpd_hip_set_shadow_jitter(on, JITTER_SEED): the counts are those of the setting
    off, since no candidate, label or draw depends on it and detect_sis keeps every hand at this min_score."""
    with ec.jitter(oracle_mod, ec.JITTER_SEED):
        _proofs(oracle_mod, name)


@pytest.mark.parametrize("name", ec.JITTER_VARIANTS)
def test_the_shadow_jitter_decides_the_scores(oracle_mod, name):
    """What tests/test_gpu_entries_by_variant_jitter.py compares is not what the walk with the setting off compares: with 15
    channels at least half of the candidates' detect scores differ; without a shadow channel none does."""
    om = oracle_mod
    off = ec.detect(om, name)
    with ec.jitter(om, ec.JITTER_SEED):
        on = ec.detect(om, name)
    assert on is not off and on["n_cand"] == off["n_cand"] > 0
    a, b = on["cands"].copy(), off["cands"].copy()
    differ = int((a["score"] != b["score"]).sum())
    print(name, "detect scores that differ with the jitter on: %d of %d" % (differ, len(a)))
    a["score"] = b["score"] = 0
    assert a.tobytes() == b.tobytes()  # the records are the same but for the score
    if ec.inputs(name, om.default_params)[0].image_num_channels == 15:
        assert 2 * differ >= len(a), (name, differ, len(a))
    else:
        assert name == "default_c12" and differ == 0 and on["hands"].tobytes() == off["hands"].tobytes()


def _proofs(om, name):
    n_cand, live, n_sis, (v_cand, v_pos, v_out) = COUNTS[name]
    p = ec.inputs(name, om.default_params)[0]
    slots = ec.slots(p)
    assert slots == {"three_axes": 24, "offlattice_three_axes": 24, "axis1_four_orientations": 4, "twelve_orientations": 12}.get(name, 8)

    # detect / detect_select
    d = ec.detect(om, name)
    assert d["hands"].shape == (rcs.NUM_SAMPLES, slots)
    assert d["n_cand"] == n_cand >= 5
    assert len(ec.selected(d, ec.SELECT_K)) == min(ec.SELECT_K, n_cand)
    if n_cand > ec.SELECT_K:  # selectGrasps reorders and drops: its result is not a prefix of the candidate list
        assert not np.array_equal(d["top"], np.arange(ec.SELECT_K))

    # the batch's second job differs from the first: another cloud, fewer samples, one camera; it has candidates of its own
    clouds, samples = ec.batch_jobs(name, om.default_params)
    assert [len(s) for s in samples] == [rcs.NUM_SAMPLES, ec.JOB1_SAMPLES, 0]
    assert clouds[0]["cam_source"].shape[0] == rcs.VARIANTS[name][2] and clouds[1]["cam_source"].shape[0] == 1
    assert not np.array_equal(clouds[0]["xyz"], clouds[1]["xyz"]) and not np.isin(samples[1], samples[0]).all()

    # images_given: the images are not empty, set (b) is another list, and for 15 channels the stream position matters
    a, b = ec.given_sets(om, name)["a"], ec.given_sets(om, name)["b"]
    ga = ec.given(om, name, "a", 0)
    assert a.shape == b.shape == (rcs.NUM_SAMPLES, slots)
    assert len(ga["cand"]) == n_cand and 0 < int(b["valid"].sum()) < n_cand
    assert np.array_equal(b["sample"], a[::-1]["sample"])
    if name not in FEW_IMAGES:
        assert ec.nonempty(ga["images"]) >= 0.9 * n_cand, (ec.nonempty(ga["images"]), n_cand)
    if p.image_num_channels == 15:
        assert ga["draws"] > 0
        assert ec.given(om, name, "a", ec.LCG_BASES[1])["images"].tobytes() != ga["images"].tobytes()
    else:
        assert ga["draws"] == 0

    # detect_sis
    s = ec.sis_predict(om, name)
    assert s["live"] == live and min(live) >= 3
    assert len(s["hands"]) == n_sis > n_cand  # the rounds add hands to the initial pass's
    assert s["samples"].shape == (ec.SIS["rounds"], ec.SIS["per"], 3) and s["consumed"].shape == (ec.SIS["rounds"], 2)
    assert s["candidates"][0] == n_cand

    # label_view
    v = ec.view(om, name)
    assert (v["num_candidates"], v["num_positives"], v["num_out"]) == (v_cand, v_pos, v_out)
    assert v["rounds_run"] == ec.VIEW_ROUNDS and v_cand >= 15 and len(v["all_labels"]) == v_cand
    assert (v["round_counts"][:, 0] > 0).all()
    if name in VIEW_KEEPS_NOTHING:
        assert v_out == 0
    else:
        assert v_out >= 2 and v_out == 2 * v_pos
