"""The host-only parts of training-set generation: gpd_hip_balance_view (DataGenerator::balanceInstances, the definition the
device selection of gpd_hip_label_view equals), the seeded shuffle, the job struct's layout, and generate_data's usage and its
failure without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import label_view_cases as lvc
from gpd_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "gpd_amd", "host", "generate_data")
MAX_GRASPS = (0, 1, 4, 5, 500)


def _label_vectors():
    rng = np.random.RandomState(20)
    out = [np.zeros(0, np.uint8)]
    for n in list(range(1, 40)) + [63, 64, 65, 100, 128, 255, 256, 299, 300]:
        for p in (0.0, 0.1, 0.5, 0.9, 1.0):  # all negative, more negatives, about equal, fewer negatives, all positive
            out.append((rng.random_sample(n) < p).astype(np.uint8))
        half = np.zeros(n, np.uint8)  # exactly equal (or one apart), positives first / last / shuffled
        half[: n // 2] = 1
        out += [half, half[::-1].copy(), rng.permutation(half)]
    return out


def test_balance_view_equals_the_restatement():
    seen = set()
    for lab in _label_vectors():
        P, N = int(lab.sum()), int(len(lab) - lab.sum())
        seen.add("more_neg" if N > P > 0 else "fewer_neg" if P > N > 0 else "equal" if P == N else "all_pos" if N == 0 else "all_neg")
        for mx in MAX_GRASPS:
            got, want = api.balance_view(lab, mx), lvc.balance(lab, mx)
            assert got.dtype == np.int32 and np.array_equal(got, want), (len(lab), mx, got, want)  # the indices and their order
            end = len(got) // 2
            assert end == min(P, N, mx // 2)
            assert lab[got[:end]].all() and not lab[got[end:]].any()  # positives first
            assert (np.diff(got[:end]) > 0).all() and (np.diff(got[end:]) > 0).all()
    assert seen == {"more_neg", "fewer_neg", "equal", "all_pos", "all_neg"}
    # any non-zero label is a positive; the counts come back as documented
    lab = np.array([0, 3, 0, 255, 0], np.uint8)
    assert api.balance_view(lab, 4).tolist() == [1, 3, 0, 2]
    n, npos = C.c_int(-1), C.c_int(-1)
    out = np.full(8, -7, np.int32)
    assert api.lib().gpd_hip_balance_view(api._ptr(lab), 5, 500, api._ptr(out), C.byref(n), C.byref(npos)) == 0
    assert (n.value, npos.value) == (4, 2) and out.tolist() == [1, 3, 0, 2, -7, -7, -7, -7]
    assert api.lib().gpd_hip_balance_view(api._ptr(lab), -1, 4, api._ptr(out), C.byref(n), C.byref(npos)) == -1
    assert api.lib().gpd_hip_balance_view(api._ptr(lab), 5, 4, None, C.byref(n), C.byref(npos)) == -1


def _shuffle_restated(seed, sizes):
    s, M, out = 0x9E3779B97F4A7C15 ^ seed, (1 << 64) - 1, []
    for n in sizes:
        order = list(range(n))
        for i in range(n - 1, 0, -1):
            s ^= (s << 13) & M
            s ^= s >> 7
            s ^= (s << 17) & M
            j = s % (i + 1)
            order[i], order[j] = order[j], order[i]
        out.append(order)
    return out


def test_shuffle_orders_is_one_seeded_stream_through_the_sets():
    sizes = [0, 1, 2, 7, 0, 64, 301]
    for seed in (0, 1, 0xFFFFFFFF):
        got = api.shuffle_orders(seed, sizes)
        assert [g.tolist() for g in got] == _shuffle_restated(seed, sizes)
        for g, n in zip(got, sizes):
            assert sorted(g.tolist()) == list(range(n))
    assert api.shuffle_orders(0, [301])[0].tolist() != api.shuffle_orders(0, sizes)[6].tolist()  # the stream runs on
    assert api.shuffle_orders(0, [50])[0].tolist() != api.shuffle_orders(1, [50])[0].tolist()


def test_job_struct_layout():
    assert api.lib().gpd_hip_sizeof_label_view_job() == C.sizeof(api.LabelViewJob) == 136
    for name in ("gpd_hip_upload_ground_truth", "gpd_hip_label_view", "gpd_hip_balance_view", "gpd_hip_sizeof_label_view_job",
                 "gpd_hip_shuffle_orders"):
        assert name in api.EXPORTS and getattr(api.lib(), name)
    f = api.LabelViewJob
    assert (f.sample_indices.offset, f.images.offset, f.capacity.offset, f.all_labels.offset, f.round_counts.offset) == (0, 24, 56, 64, 80)
    assert (f.rounds_run.offset, f.gt_neighbourhoods.offset, f.d2h_bytes.offset, f.stage_ms.offset) == (88, 108, 112, 120)


def test_generate_data_usage_and_no_gpu_fails_loudly(tmp_path):
    assert os.path.exists(CLI), "run __graft_entry__.build()"
    out = subprocess.run([CLI], capture_output=True, text=True)
    assert out.returncode != 0 and "Usage: generate_data CONFIG_FILE" in out.stdout
    import torch
    if torch.cuda.is_available():
        return
    (tmp_path / "objects.txt").write_text("thing\n")
    cfg = tmp_path / "generate_data.cfg"
    cfg.write_text("data_root = %s/\nobjects_file_location = %s/objects.txt\noutput_root = %s/\nnum_views_per_object = 1\n"
                   "image_num_channels = 15\n" % (tmp_path, tmp_path, tmp_path))
    out = subprocess.run([CLI, str(cfg)], capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode != 0 and "ERROR" in out.stdout  # no device -> error, not an empty data set
    assert not (tmp_path / "train_images.npy").exists()
