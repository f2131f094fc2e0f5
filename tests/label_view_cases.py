"""What gpd_hip_label_view must return, composed from the oracle's own entries (tests/test_gpu_label_view.py and the CLI test share
it): per round oracle.search -> oracle.filter_workspace -> oracle.images give the candidates and their images,
oracle.reevaluate on the ground truth gives labels and flags; the selection rule (DataGenerator::balanceInstances + the order
addInstances writes) is restated here in a few lines."""
import numpy as np

import ref_cases as rcs


def balance(labels, max_grasps_per_view):
    """Indices kept of a view's accumulated labels: the first `end` positives, then the first `end` negatives."""
    labels = np.asarray(labels).reshape(-1)
    pos, neg = np.flatnonzero(labels != 0), np.flatnonzero(labels == 0)
    end = min(len(pos), len(neg), max(int(max_grasps_per_view), 0) // 2)
    return np.concatenate([pos[:end], neg[:end]]).astype(np.int32)


def expected_view(om, op, xyz, normals, cam, vp, gt_xyz, gt_normals, sample_rounds, min_positives, max_grasps_per_view):
    """-> dict with the fields Context.label_view returns (those an oracle can know), plus `sets_with_candidates` per round and
    `search_flags`: the accumulated candidates' full_antipodal flags as the SEARCH left them (before the ground-truth check)."""
    Cn = op.image_num_channels
    sample_rounds = np.asarray(sample_rounds, np.int32)
    sample_rounds = sample_rounds.reshape(len(sample_rounds), -1)
    imgs, recs, labs, flags, counts, live = [], [], [], [], np.zeros((len(sample_rounds), 2), np.int32), []
    positives, r = 0, 0
    while r < len(sample_rounds) and positives < min_positives:
        hands = om.search(op, xyz, normals, sample_rounds[r])
        if len(hands):
            hands = om.filter_workspace(op, hands)
            img, cand = om.images(op, xyz, normals, cam, vp, hands)
            cr = hands.reshape(-1)[cand].copy()
            if len(cr):
                flags.append(cr["full_antipodal"].copy())
                lab, cr = om.reevaluate(op, gt_xyz, gt_normals, cr)
                imgs.append(img)
                recs.append(cr)
                labs.append(lab.astype(np.uint8))
                counts[r] = (len(cr), int(lab.sum()))
                positives += int(lab.sum())
                live.append(len(np.unique(cr["set_index"])))
        r += 1
    n = int(counts[:, 0].sum())
    all_img = np.concatenate(imgs) if imgs else np.zeros((0, 60, 60, Cn), np.uint8)
    all_rec = np.concatenate(recs) if recs else np.zeros(0, om.HAND_DTYPE)
    all_lab = np.concatenate(labs) if labs else np.zeros(0, np.uint8)
    keep = balance(all_lab, max_grasps_per_view)
    return dict(images=all_img[keep], labels=all_lab[keep], hands=all_rec[keep], src_index=keep, rounds_run=r, num_candidates=n,
                num_positives=positives, num_out=len(keep), num_positives_out=len(keep) // 2, round_counts=counts, all_labels=all_lab,
                sets_with_candidates=live, search_flags=np.concatenate(flags) if flags else np.zeros(0, np.uint8),
                all_images=all_img, all_hands=all_rec)


def assert_view(got, want, what=""):
    """Byte for byte: counters, images, labels, the whole record array, src_index, round_counts, all_labels when present."""
    for k in ("rounds_run", "num_candidates", "num_positives", "num_out", "num_positives_out"):
        assert got[k] == want[k], (what, k, got[k], want[k], got["round_counts"].tolist(), want["round_counts"].tolist())
    assert np.array_equal(got["round_counts"], want["round_counts"]), (what, got["round_counts"].tolist(), want["round_counts"].tolist())
    assert np.array_equal(got["src_index"], want["src_index"]), (what, got["src_index"], want["src_index"])
    assert got["labels"].dtype == np.uint8 and np.array_equal(got["labels"], want["labels"]), what
    bad = rcs.records_equal(got["hands"], want["hands"])
    assert not bad, (what, bad)
    assert got["hands"].tobytes() == want["hands"].tobytes(), (what, [f for f in got["hands"].dtype.names
                                                                      if not np.array_equal(got["hands"][f], want["hands"][f])])
    assert np.array_equal(got["labels"], got["hands"]["full_antipodal"]), what
    assert got["images"].shape == want["images"].shape and got["images"].dtype == np.uint8, (what, got["images"].shape, want["images"].shape)
    assert got["images"].tobytes() == want["images"].tobytes(), (what, np.flatnonzero((got["images"] != want["images"]).reshape(len(want["images"]), -1).any(axis=1)))
    if "all_labels" in got:
        assert np.array_equal(got["all_labels"], want["all_labels"]), what
