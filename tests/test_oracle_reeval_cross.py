"""The oracle's HandSearch::reevaluateHypotheses against tests/pyref_hands.reevaluate, an independent numpy restatement
(cKDTree neighbourhoods with FLANN's float test, cropByHandHeight's padded list materialised), on hands of several
parameter variants re-evaluated on their own cloud and on a jittered, subsampled "ground truth" of it."""
import numpy as np
import pytest

import pyref_hands
import ref_cases as rcs


def edge_records(hands, nfp):
    """Valid hands made into the edges of the label path: no finger placement, one beyond the last, no point in reach."""
    e = hands[hands["valid"].astype(bool)][:6].copy()
    e["half_antipodal"] = 1
    e["full_antipodal"] = 1
    e["finger_placement_index"][0] = -1
    e["finger_placement_index"][1] = nfp
    e["finger_placement_index"][2] = nfp + 7
    e["sample"][3] += 5.0
    return e


@pytest.mark.parametrize("variant", ["default_c15", "deep_hand", "six_placements_wide_fingers", "friction_viable_aperture",
                                     "no_deepen", "offlattice_three_axes"])
def test_reevaluate_matches_independent_restatement(oracle_mod, variant):
    p, cl, si, _, _ = rcs.case_inputs(variant, oracle_mod.default_params)
    hands = oracle_mod.search(p, cl["xyz"], cl["normals"], si).reshape(-1)
    gt, gn, _ = rcs.ground_truth(cl["xyz"], cl["normals"], 7)
    recs = np.concatenate([hands, edge_records(hands, p.num_finger_placements)])
    total = ones = 0
    for xyz, nrm in ((cl["xyz"], cl["normals"]), (gt, gn)):
        wl, wout = oracle_mod.reevaluate(p, xyz, nrm, recs)
        gl, ghalf, gfull = pyref_hands.reevaluate(p, xyz, nrm, recs)
        assert np.array_equal(wl, gl), np.flatnonzero(wl != gl)
        assert np.array_equal(wout["half_antipodal"].astype(bool), ghalf)
        assert np.array_equal(wout["full_antipodal"].astype(bool), gfull)
        assert not wl[-6:-2].any() and not wout[-6:-2]["half_antipodal"].any() and not wout[-6:-2]["full_antipodal"].any()
        total += len(wl)
        ones += int(wl.sum())
    assert 0 < ones < total
