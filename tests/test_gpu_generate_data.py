"""generate_data (gpd::DataGenerator over gpd_hip_label_view) against the same sequence composed through gpd_amd.api:
preprocess_cloud, estimate_normals, upload_ground_truth, sample_positions, label_view and the seeded shuffle.  A temporary data
set of two objects x three views is written as ASCII PCD from seeded synthetic clouds."""
import os
import subprocess

import numpy as np
import pytest

from gpd_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "gpd_amd", "host", "generate_data")
OBJECTS, VIEWS, TEST_VIEWS = ("box_a", "can_b"), 3, (1,)
NUM_SAMPLES, MIN_GRASPS, MAX_GRASPS, MAX_ROUNDS, VOXEL, RADIUS = 12, 30, 24, 6, 0.003, 0.01
SAMPLE_SEED, SHUFFLE_SEED, CHANNELS = 5, 9, 3


def _write_pcd(path, xyz):
    """ASCII PCD, 9 significant digits: float32 round-trips exactly."""
    with open(str(path), "w") as f:
        f.write("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\n"
                "WIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA ascii\n" % (len(xyz), len(xyz)))
        for p in xyz:
            f.write("%.9g %.9g %.9g\n" % (p[0], p[1], p[2]))


def _box(rng, half, n):
    """n points on the six faces of a box around the origin, uniform by area."""
    half = np.asarray(half)
    areas = np.array([half[1] * half[2], half[0] * half[2], half[0] * half[1]]).repeat(2)
    face = rng.choice(6, size=n, p=areas / areas.sum())
    p = (rng.rand(n, 3) * 2 - 1) * half
    p[np.arange(n), face // 2] = np.where(face % 2 == 0, 1.0, -1.0) * half[face // 2]
    return p


def _cylinder(rng, r, h, n):
    """n points on the side and both caps of a cylinder around the origin, axis z."""
    a_side, a_cap = 2 * np.pi * r * h, np.pi * r * r
    part = rng.choice(3, size=n, p=np.array([a_side, a_cap, a_cap]) / (a_side + 2 * a_cap))
    th, rr = rng.rand(n) * 2 * np.pi, np.where(part == 0, r, r * np.sqrt(rng.rand(n)))
    z = np.where(part == 0, (rng.rand(n) - 0.5) * h, np.where(part == 1, h / 2, -h / 2))
    return np.stack([rr * np.cos(th), rr * np.sin(th), z], 1)


def _data_set(tmp, channels=CHANNELS, extra=""):
    """(`channels`: image_num_channels of the cfg file; `extra`: further cfg lines.)
    Per object a complete surface as the mesh and three views of it (seeded subsets, a little noise).  The objects stand on the
    camera axis, half a metre from the view point (0, 0, 0): normals flipped towards it point INTO such an object on every side,
    which is why the reference's cfg reverses them — and only then do opposite faces carry opposite normals, i.e. positives."""
    clouds = {}
    for o, name in enumerate(OBJECTS):
        rng = np.random.RandomState(40 + o)
        shape = _box(rng, (0.02, 0.03, 0.05), 5000) if o == 0 else _cylinder(rng, 0.025, 0.10, 5000)
        mesh = (shape + np.array([0.004 * o, -0.003, -0.5])).astype(np.float32)
        _write_pcd(tmp / (name + "_gt.pcd"), mesh)
        views = []
        for j in range(VIEWS):
            rng = np.random.RandomState(1000 * o + j)
            keep = np.sort(rng.choice(len(mesh), 4000, replace=False))
            v = (mesh[keep].astype(np.float64) + rng.uniform(-0.0003, 0.0003, (len(keep), 3))).astype(np.float32)
            _write_pcd(tmp / ("%s_%d.pcd" % (name, j + 1)), v)
            views.append(v)
        clouds[name] = (mesh, views)
    (tmp / "objects.txt").write_text("".join(n + "\n" for n in OBJECTS))
    out = tmp / "out"
    out.mkdir()
    cfg = tmp / "generate_data.cfg"
    cfg.write_text("# in the format of cfg/generate_data.cfg\n"
                   "data_root = %s/\nobjects_file_location = %s/objects.txt\noutput_root = %s/\n"
                   "num_views_per_object = %d\nmin_grasps_per_view = %d\nmax_grasps_per_view = %d\ntest_views = %s\n"
                   "num_samples = %d\nremove_nans = 1\nvoxel_size_views = %g\nnormals_radius = %g\nreverse_mesh_normals = 1\n"
                   "reverse_view_normals = 1\nsample_seed = %d\nshuffle_seed = %d\nmax_rounds_per_view = %d\n"
                   "image_num_channels = %d\nnum_orientations = 8\nhand_axes = 2\nworkspace_grasps = -1 1 -1 1 -1 1\n%s"
                   % (tmp, tmp, out, VIEWS, MIN_GRASPS, MAX_GRASPS, " ".join(map(str, TEST_VIEWS)), NUM_SAMPLES, VOXEL, RADIUS,
                      SAMPLE_SEED, SHUFFLE_SEED, MAX_ROUNDS, channels, extra))
    return cfg, out, clouds


def _composed(clouds, channels=CHANNELS, jitter_seed=None, per_view=True):
    """The same data set through gpd_amd.api -> (train images, train labels, test images, test labels).  With `jitter_seed` S
    every view is labelled under set_shadow_jitter(True, S + the view's ordinal in the data set), as DataGenerator::labelView
    sets it (`per_view` False: under S itself, which the generator does NOT do)."""
    ctx = api.Context(api.default_params(channels))
    sets = {"train": ([], []), "test": ([], [])}
    sizes, stored = [], []
    try:
        for o, name in enumerate(OBJECTS):
            mesh, views = clouds[name]
            ctx.upload_cloud(mesh, np.zeros_like(mesh))
            ctx.upload_ground_truth(mesh, -ctx.estimate_normals(RADIUS))
            per_object = {"train": ([], []), "test": ([], [])}
            for j, v in enumerate(views):
                xyz, cam, _, _ = ctx.preprocess_cloud(v, np.ones((1, len(v)), np.int32), None, VOXEL)
                ctx.upload_cloud(xyz, np.zeros_like(xyz), cam, np.zeros((1, 3)))
                ctx.upload_cloud(xyz, -ctx.estimate_normals(RADIUS), cam, np.zeros((1, 3)))
                seed = (SAMPLE_SEED + 1000003 * (o * VIEWS + j)) & 0xFFFFFFFF
                rounds = np.stack([api.sample_positions(len(xyz), NUM_SAMPLES, (seed + r) & 0xFFFFFFFF) for r in range(MAX_ROUNDS)])
                if jitter_seed is not None:
                    ctx.set_shadow_jitter(True, jitter_seed + (o * VIEWS + j if per_view else 0))
                got = ctx.label_view(rounds, MIN_GRASPS, MAX_GRASPS)
                which = per_object["test" if j in TEST_VIEWS else "train"]
                which[0].append(got["images"])
                which[1].append(got["labels"])
            for k in ("train", "test"):
                img, lab = np.concatenate(per_object[k][0]), np.concatenate(per_object[k][1])
                sizes.append(len(lab))
                stored.append((k, img, lab))
        for (k, img, lab), order in zip(stored, api.shuffle_orders(SHUFFLE_SEED, sizes)):
            sets[k][0].append(img[order])
            sets[k][1].append(lab[order])
    finally:
        ctx.close()
    return tuple(np.concatenate(sets[k][i]) for k in ("train", "test") for i in (0, 1))


def test_generate_data_cli_equals_the_composed_sequence(tmp_path):
    assert os.path.exists(CLI), "run __graft_entry__.build()"
    cfg, out_dir, clouds = _data_set(tmp_path)
    out = subprocess.run([CLI, str(cfg)], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    want = _composed(clouds)
    names = ("train_images", "train_labels", "test_images", "test_labels")
    got = [np.load(str(out_dir / (n + ".npy"))) for n in names]
    for n, g, w in zip(names, got, want):
        shape = (len(w), 60, 60, CHANNELS) if n.endswith("images") else (len(w), 1)
        assert g.dtype == np.uint8 and g.shape == shape, (n, g.dtype, g.shape, shape)
        assert np.array_equal(g.reshape(w.shape), w), n
        with open(str(out_dir / (n + ".npy")), "rb") as f:
            assert f.read(8) == b"\x93NUMPY\x01\x00"  # format 1.0
    n_train, n_test = len(want[1]), len(want[3])
    assert n_train > 0 and n_test > 0 and 0 < int(want[1].sum()) < n_train  # both classes, balanced
    rounds = [int(l.split()[1].rstrip(",")) for l in out.stdout.splitlines() if l.startswith("rounds: ")]
    assert len(rounds) == len(OBJECTS) * VIEWS and max(rounds) > 1, rounds  # some view needed more than one round
    assert int(want[1].sum()) * 2 == n_train and int(want[3].sum()) * 2 == n_test
    assert "Generated %d training and test %d instances" % (n_train, n_test) in out.stdout
    assert out.stdout.count("positives, negatives found for this view:") == len(OBJECTS) * VIEWS
    assert out.stdout.count("test view, # test data:") == len(OBJECTS) * len(TEST_VIEWS)


JITTER_SEED = 0x5EED5EED5EED


def test_generate_data_cli_at_15_channels_with_a_shadow_jitter_seed_per_view(tmp_path):
    """hip_shadow_jitter = 1 in the cfg file, 15 channels: DataGenerator gives every view the seed S + object *
    num_views_per_object + view (data_generator.cpp, labelView).  The files equal the sequence composed with those seeds byte for
    byte, and not the one composed with S for every view, nor the one with the setting off."""
    cfg, out_dir, clouds = _data_set(tmp_path, 15, "hip_shadow_jitter = 1\nhip_shadow_jitter_seed = %d\n" % JITTER_SEED)
    out = subprocess.run([CLI, str(cfg)], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "hip_shadow_jitter: 1" in out.stdout and ("hip_shadow_jitter_seed: %d" % JITTER_SEED) in out.stdout
    want = _composed(clouds, 15, JITTER_SEED)
    names = ("train_images", "train_labels", "test_images", "test_labels")
    got = [np.load(str(out_dir / (n + ".npy"))) for n in names]
    for n, g, w in zip(names, got, want):
        shape = (len(w), 60, 60, 15) if n.endswith("images") else (len(w), 1)
        assert g.dtype == np.uint8 and g.shape == shape, (n, g.dtype, g.shape, shape)
        assert g.tobytes() == w.tobytes(), n
    n_train, n_test = len(want[1]), len(want[3])
    assert n_train > 0 and n_test > 0 and 0 < int(want[1].sum()) < n_train
    shadow = [4, 9, 14]
    assert all((want[0][..., c] > 0).any() for c in shadow)
    # the labels and the twelve other channels do not depend on the seeds; the shadow channels of the training views do
    for other in (_composed(clouds, 15, JITTER_SEED, per_view=False), _composed(clouds, 15)):
        assert other[0].shape == want[0].shape and np.array_equal(other[1], want[1])
        rest = [c for c in range(15) if c not in shadow]
        assert other[0][..., rest].tobytes() == want[0][..., rest].tobytes()
        assert other[0][..., shadow].tobytes() != want[0][..., shadow].tobytes()
