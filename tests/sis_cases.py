"""What gpd_hip_detect_sis must return, composed from the oracle's own entries and the Python restatement of the draws
(tests/pyref_sis.py); tests/test_gpu_detect_sis.py and tests/test_host_sis_resident.py share it.

replay():  the samples of a run (the initial indices, every round's coordinates) through oracle.search / search_xyz ->
           filter_workspace -> the live hand sets concatenated -> ONE oracle.images + oracle.lenet over all -> score > min_score ->
           oracle.find_clusters.
predict(): the same with the samples of every round drawn by pyref_sis from the live centres the oracle found so far: the
           whole call without the library, which is how the seeds of the tests were picked on the CPU."""
import numpy as np

import pyref_sis
import ref_cases as rcs
from gpd_amd import synth

CLOUD_SEED, CLOUD_POINTS, N_INIT, ROUNDS, PER = 99, 12000, 40, 3, 40
PROB_RAND, SIGMA, MIN_SCORE = 0.3, 0.02, -300.0
WS_ALL = (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0)
SEED = {0: 7, 1: 7}  # per sampling method: picked with predict() so that the oracle alone meets the tests' conditions

_scene = {}


def scene(cams=2):
    """(cloud dict, cam_source, view_points, initial sample indices) of the base case."""
    if cams not in _scene:
        cl = synth.make_cloud(CLOUD_SEED, CLOUD_POINTS)
        if cams == 2:
            cam, vp = rcs._cams(2, len(cl["xyz"]))
        else:
            cam, vp = cl["cam_source"], cl["view_points"]
        _scene[cams] = (cl, cam, vp, synth.sample_indices(cl, N_INIT).astype(np.int32))
    return _scene[cams]


def live_sets(om, p, hands):
    if not len(hands):
        return hands
    hands = om.filter_workspace(p, hands.copy())
    return hands[hands["valid"].astype(bool).any(axis=1)]


def finish(om, p, cl, cam, vp, sets, weights, min_score, min_inliers, remove_inliers=False):
    """The tail over the live hand sets of all passes -> dict(hands, all_hands, scores, centres, live, candidates)."""
    live = [len(s) for s in sets]
    cands = [int(s["valid"].astype(bool).sum()) for s in sets]
    nonempty = [s for s in sets if len(s)]
    if not nonempty:
        z = np.zeros(0, om.HAND_DTYPE)
        return dict(hands=z, all_hands=z, centres=np.zeros((0, 3)), live=live, candidates=cands)
    allh = np.concatenate(nonempty)
    img, cand = om.images(p, cl["xyz"], cl["normals"], cam, vp, allh)
    allh["set_index"] = np.arange(len(allh), dtype=np.int32)[:, None]  # the index in the accumulated live list
    sc = om.lenet(img, weights)
    recs = allh.reshape(-1)[cand].copy()
    recs["score"] = sc
    want = recs[sc > np.float64(min_score)]
    if min_inliers > 0 and len(want):
        want, _, _ = om.find_clusters(want, want["score"].astype(np.float64), min_inliers, remove_inliers)
    return dict(hands=want, all_hands=recs, centres=allh[:, 0]["sample"].copy(), live=live, candidates=cands)


def replay(om, p, cl, cam, vp, init, rounds, weights, min_score=MIN_SCORE, min_inliers=0, remove_inliers=False):
    sets = [live_sets(om, p, om.search(p, cl["xyz"], cl["normals"], init))]
    for r in rounds:
        sets.append(live_sets(om, p, om.search_xyz(p, cl["xyz"], cl["normals"], r)))
    return finish(om, p, cl, cam, vp, sets, weights, min_score, min_inliers, remove_inliers)


def predict(om, p, cl, cam, vp, init, weights, seed, method, rounds=ROUNDS, per=PER, prob=PROB_RAND, sigma=SIGMA, workspace=WS_ALL,
            min_score=MIN_SCORE, min_inliers=0, uniform_list="init"):
    """-> finish()'s dict plus samples [rounds_run, per, 3] and consumed [rounds_run, 2]."""
    sets = [live_sets(om, p, om.search(p, cl["xyz"], cl["normals"], init))]
    samples, consumed = [], []
    lst = init if uniform_list == "init" else uniform_list
    for r in range(rounds):
        centres = np.concatenate([s[:, 0]["sample"] for s in sets if len(s)]) if any(len(s) for s in sets) else np.zeros((0, 3))
        if not len(centres):
            break
        st = pyref_sis.draw_round(seed, r, centres, lst, cl["xyz"], workspace, method, per, prob, sigma)
        samples.append(st["samples"])
        consumed.append(st["consumed"])
        sets.append(live_sets(om, p, om.search_xyz(p, cl["xyz"], cl["normals"], st["samples"])))
    out = finish(om, p, cl, cam, vp, sets, weights, min_score, min_inliers)
    out["samples"] = np.array(samples).reshape(-1, per, 3)
    out["consumed"] = np.array(consumed, np.int32).reshape(-1, 2)
    return out


def centres_before(round_counts):
    """Live centres accumulated before every round (row 0 of round_counts is the initial pass) -> list, one per round."""
    return np.cumsum(np.asarray(round_counts)[:, 0])[:-1].tolist()
