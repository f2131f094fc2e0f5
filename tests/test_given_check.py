"""gpd_hip_given_check (gpd_amd/csrc/given_model.h), host only: which caller-supplied hand sets gpd_hip_images_given and
gpd_hip_score_given take.  It must accept every record a search returns, and refuse — naming the set and the slot — a record
whose box the image kernels' voxel windows were not sized for, whose frame is no rotation or whose sample is not its set's."""
import numpy as np
import pytest

import given_cases as gc
from gpd_amd import api


@pytest.fixture(scope="module")
def searched(oracle_mod):
    cl, si = gc.scene()
    op = oracle_mod.default_params(15)
    hands = oracle_mod.filter_workspace(op, oracle_mod.search(op, cl["xyz"], cl["normals"], si))
    assert hands.shape == (gc.NUM_SAMPLES, 8) and 0 < int(hands["valid"].sum()) < hands.size
    return cl, si, hands


def test_accepts_what_a_search_returns(searched):
    _, _, hands = searched
    p = api.default_params(15)
    assert api.given_check(p, hands) is None
    # ... whatever the image layout and before the workspace filter's flags as well
    assert api.given_check(api.default_params(3), hands) is None
    # the slack is there for records like these: the search leaves bottom a rounding error below or above zero
    b = hands["bottom"][hands["valid"].astype(bool)]
    print("bottom of the searched hands: min %.3g max %.3g; |center| max %.3g" % (b.min(), b.max(), np.abs(hands["center"]).max()))
    assert b.max() <= 1e-9 and b.min() >= p.init_bite - p.hand_depth - 1e-9
    assert api.given_check(p, hands[:0]) is None


def test_accepts_foreign_hands_and_garbage_husks(searched):
    cl, si, hands = searched
    p = api.default_params(15)
    f, off, far = gc.foreign(hands, cl["normals"][si])
    assert len(off) >= 5 and len(far) >= 3 and int(f["valid"].sum()) >= 100
    assert api.given_check(p, f) is None
    g = gc.husks_with_garbage(f)
    assert g.tobytes() != f.tobytes() and np.isnan(g["bottom"]).any()
    assert api.given_check(p, g) is None


def test_refuses_and_names_the_record(searched):
    _, _, hands = searched
    p = api.default_params(15)
    cases = gc.refusals(hands, p)
    assert [c[0] for c in cases] == ["nan_sample", "sample_one_ulp", "frame_scaled", "bottom_above", "bottom_below", "center_over",
                                     "center_under"]
    for name, h, s, j in cases:
        got = api.given_check(p, h)
        assert got is not None, name
        assert got[:2] == (s, j), (name, got, s, j)
        assert "set %d, slot %d" % (s, j) in got[2], got[2]
        # the C entry itself: GPD_ERR_INVALID (-1 is not assumed: whatever the header's constant is, it is not 0), NULL outputs allowed
        rc = api.lib().gpd_hip_given_check(p, h.ctypes.data, h.shape[0], None, None)
        assert rc != 0
    # the first offending record is reported: two bad records, the earlier one named
    h = cases[3][1].copy()
    s_lo, j_lo = cases[2][2], cases[2][3]
    h["frame"][s_lo, j_lo] *= 1.0 + 1e-5
    first = min((cases[3][2], cases[3][3]), (s_lo, j_lo))
    assert api.given_check(p, h)[:2] == first


def test_inside_the_slack_is_accepted(searched):
    _, _, hands = searched
    p = api.default_params(15)
    s, j = np.argwhere(hands["valid"].astype(bool))[0]
    bound = 0.5 * (p.hand_outer_diameter - p.finger_width)
    for field, value in (("bottom", 5e-10), ("bottom", p.init_bite - p.hand_depth - 5e-10), ("center", bound + 5e-10),
                         ("center", -bound - 5e-10), ("bottom", -6.9e-18)):
        h = hands.copy()
        h[field][s, j] = value
        assert api.given_check(p, h) is None, (field, value)
    h = hands.copy()
    h["frame"][s, j] *= 1.0 + 1e-7  # F^T F - I = 2e-7 on the diagonal: inside 1e-6
    assert api.given_check(p, h) is None
