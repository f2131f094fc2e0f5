"""What an entry answers when it is called out of order: no cloud uploaded, no LeNet weights set, no ground truth uploaded.  The
return code and the exact text of each, as the library has given them since the entries exist; every refusal happens on the host
before anything is enqueued, and leaves nothing behind: the refused context goes on to detect and to score.

An entry that needs both a cloud and weights names the one it looks at first: the fused detects and detect_sis the weights,
score_given the cloud.  So "no cloud uploaded" is asked of all eleven entries on a context that has its weights, and a context
with nothing at all is asked what each entry says first."""
import numpy as np
import pytest

import entry_cases as ec
from gpd_amd import api

pytestmark = pytest.mark.gpu

NAME = "default_c1"  # one channel: the smallest images of tests/ref_cases.py (8000 points, 24 samples)
STATE = -4           # GPD_ERR_STATE
NO_CLOUD, NO_WEIGHTS = "no cloud uploaded", "LeNet weights not set"
NO_GROUND_TRUTH = "no ground truth uploaded (gpd_hip_upload_ground_truth)"


def _calls(ctx, si, cl, sets):
    """entry name -> the call, on inputs that are in order themselves."""
    rounds = ec.view_rounds(NAME)
    return {
        "detect": lambda: ctx.detect(si),
        "detect_samples": lambda: ctx.detect_samples(cl["xyz"][si]),
        "detect_select": lambda: ctx.detect_select(si, ec.SELECT_K),
        "search": lambda: ctx.search(si),
        "search_samples": lambda: ctx.search_samples(cl["xyz"][si]),
        "reevaluate": lambda: ctx.reevaluate(sets.reshape(-1)),
        "images": lambda: ctx.images(sets),
        "images_given": lambda: ctx.images_given(sets),
        "score_given": lambda: ctx.score_given(sets),
        "label_view": lambda: ctx.label_view(rounds, ec.MIN_POSITIVES, ec.MAX_GRASPS_PER_VIEW),
        "detect_sis": lambda: ctx.detect_sis(si, 1, 8),
        "score": lambda: ctx.score(np.zeros((2, 60, 60, ctx.params.image_num_channels), np.uint8)),
    }


def _refused(calls, entry, text):
    with pytest.raises(api.GpdHipError) as e:
        calls[entry]()
    assert str(e.value) == "libgpd_hip error %d: gpd_hip_%s: %s" % (STATE, entry, text), (entry, str(e.value))


def test_refusals_by_state_and_the_context_works_afterwards():
    p, cl, si, w = ec.inputs(NAME, api.default_params)
    blank = np.zeros((2, ec.slots(p)), api.HAND_DTYPE)  # no valid hand: enough for a call that is refused before it reads them
    cloudless = ["detect", "detect_samples", "detect_select", "search", "search_samples", "reevaluate", "images", "images_given",
                 "score_given", "label_view", "detect_sis"]
    weights_first = ["detect", "detect_samples", "detect_select", "detect_sis"]
    ctx, armed = api.Context(p), api.Context(p)
    try:
        # ---- weights, no cloud: every entry that reads the cloud says so ----
        armed.set_lenet_weights(w)
        calls = _calls(armed, si, cl, blank)
        for entry in cloudless:
            _refused(calls, entry, NO_CLOUD)

        # ---- nothing at all: the entries that score look at the weights first, the others at the cloud ----
        calls = _calls(ctx, si, cl, blank)
        for entry in cloudless:
            _refused(calls, entry, NO_WEIGHTS if entry in weights_first else NO_CLOUD)
        _refused(calls, "score", NO_WEIGHTS)

        # ---- a cloud, no weights, no ground truth ----
        ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
        sets = ctx.search(si)
        assert len(sets) > 0 and sets["valid"].any()
        calls = _calls(ctx, si, cl, sets)
        for entry in ["detect", "detect_select", "detect_sis", "score_given", "score"]:
            _refused(calls, entry, NO_WEIGHTS)
        _refused(calls, "label_view", NO_GROUND_TRUTH)

        # ---- the weights arrive: the refusals left no state behind ----
        ctx.set_lenet_weights(w)
        hands, n_sets, n_cand = ctx.detect_select(si, ec.SELECT_K)
        assert n_sets > 0 and n_cand > 0 and len(hands) == min(ec.SELECT_K, n_cand)
        scored, scores, cand, _ = ctx.score_given(sets)
        assert len(scores) == len(cand) == int(sets["valid"].astype(bool).sum()) and np.isfinite(scores).all()
        assert np.array_equal(scored.reshape(-1)["score"][cand], scores)
    finally:
        ctx.close()
        armed.close()
