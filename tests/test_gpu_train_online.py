"""Resident training sets as pools that grow, and gpd_hip_train_append_view: a view's kept instances gathered straight into a
pool.  Every comparison is byte for byte; the yardstick is the route that already exists — Context.label_view, Trainer.set_data.
There are no tolerances."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ref_cases as rcs
from gpd_amd import api
from test_gpu_label_view import _context, _rounds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {15: "default_c15", 3: "default_c3", 1: "default_c1"}
COUNTERS = ("rounds_run", "num_candidates", "num_positives", "num_out", "num_positives_out", "gt_neighbourhoods")
IMAGE_BYTES_15 = 3600 * 15

_ref = {}


def _label_view(channels, max_grasps, rounds=6):
    """What Context.label_view returns for the case: computed once per setting, shared by the tests, never modified."""
    key = (channels, max_grasps, rounds)
    if key not in _ref:
        ctx, cl = _context(CASES[channels])
        try:
            _ref[key] = ctx.label_view(_rounds(cl, 6)[:rounds], 3, max_grasps, want_all_labels=True)
        finally:
            ctx.close()
    return _ref[key]


def _random_set(channels, n, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (n, 60, 60, channels)).astype(np.uint8), rng.randint(0, 2, n).astype(np.uint8)


def _assert_appended(got, want, t, which, all_labels=True):
    for k in COUNTERS:
        assert got[k] == want[k], (k, got[k], want[k])
    assert np.array_equal(got["round_counts"], want["round_counts"])
    if all_labels:
        assert got["all_labels"].tobytes() == want["all_labels"].tobytes()
    img, lab = t.get_data(got["first"], got["num_out"], which=which)
    assert img.tobytes() == want["images"].tobytes()
    assert lab.tobytes() == want["labels"].tobytes()
    bound = 64 * got["rounds_run"] + (len(got["all_labels"]) if all_labels else 0) + 4096
    print("append_view: %d kept of %d candidates, %d bytes to the host (bound %d, one image %d), stage ms %s"
          % (got["num_out"], got["num_candidates"], got["d2h_bytes"], bound, img[0].size if len(img) else 0, ["%.3f" % m for m in got["stage_ms"]]))
    assert 0 <= got["d2h_bytes"] <= bound, (got["d2h_bytes"], bound)


# ---- 1. a view lands in the pool as label_view returns it --------------------------------------------------------------------
# 16-byte units per image: C = 15: 3375 = 13 * 256 + 47, C = 3: 675 (a tail in the last workgroup), C = 1: 225 (less than one)
@pytest.mark.parametrize("channels", [15, 3, 1])
@pytest.mark.parametrize("max_grasps, num_out", [(4, 4), (5, 4), (500, 6)])
def test_a_view_lands_in_the_pool(channels, max_grasps, num_out):
    want = _label_view(channels, max_grasps)
    if channels == 15:  # the counts tests/test_gpu_label_view.py pins for this case
        assert (want["num_candidates"], want["num_out"]) == (128, num_out)
    assert want["num_out"] > 0
    pre_img, pre_lab = _random_set(channels, 2, 5)
    ctx, cl = _context(CASES[channels])
    try:
        t = api.Trainer(ctx)
        try:
            assert t.count() == (0, 0)
            assert t.append_data(pre_img, pre_lab) == 0
            got = t.append_view(ctx, _rounds(cl, 6), 3, max_grasps, want_all_labels=True)
            assert got["first"] == 2 and t.count()[0] == 2 + want["num_out"]
            _assert_appended(got, want, t, 0)
            img, lab = t.get_data(0, 2)
            assert img.tobytes() == pre_img.tobytes() and lab.tobytes() == pre_lab.tobytes()
            # the second set, without all_labels
            got = t.append_view(ctx, _rounds(cl, 6), 3, max_grasps, which=1)
            assert got["first"] == 0 and "all_labels" not in got and t.count(1)[0] == want["num_out"]
            _assert_appended(got, want, t, 1, all_labels=False)
        finally:
            t.close()
    finally:
        ctx.close()


# ---- 2. nothing kept ---------------------------------------------------------------------------------------------------------
def test_nothing_kept():
    pre_img, pre_lab = _random_set(15, 5, 6)
    ctx, cl = _context(CASES[15])
    try:
        t = api.Trainer(ctx)
        try:
            t.set_state(api.init_state(15, 2))
            t.append_data(pre_img, pre_lab)
            before = t.count()
            got = t.append_view(ctx, _rounds(cl, 6)[:1], 3, 500, want_all_labels=True)  # round 0: 24 candidates, no positive
            assert (got["rounds_run"], got["num_candidates"], got["num_positives"], got["num_out"]) == (1, 24, 0, 0)
            assert got["first"] == 5 and t.count() == before
            img, lab = t.get_data()
            assert img.tobytes() == pre_img.tobytes() and lab.tobytes() == pre_lab.tobytes()
            losses = t.steps(np.arange(5, dtype=np.int32)[None, :])
            assert losses.shape == (1,) and np.isfinite(losses).all()
        finally:
            t.close()
    finally:
        ctx.close()


# ---- 3. growth in the middle -------------------------------------------------------------------------------------------------
def test_growth_in_the_middle():
    want = _label_view(3, 500)
    k = want["num_out"]
    pre_img, pre_lab = _random_set(3, 7, 7)
    more_img, more_lab = _random_set(3, 4, 8)
    ctx, cl = _context(CASES[3])
    try:
        t = api.Trainer(ctx)
        try:
            t.set_data(pre_img, pre_lab)  # a set made by set_data can be appended to
            assert t.count() == (7, 7)
            t.reserve(7 + k - 1)
            assert t.count() == (7, 7 + k - 1)
            got = t.append_view(ctx, _rounds(cl, 6), 3, 500, want_all_labels=True)
            assert got["first"] == 7
            n, cap = t.count()
            assert n == 7 + k and cap >= n
            _assert_appended(got, want, t, 0)
            # the same through append_data: one image short again
            t.reserve(n + len(more_lab) - 1)
            assert t.count() == (n, n + len(more_lab) - 1)
            assert t.append_data(more_img, more_lab) == n
            n2, cap2 = t.count()
            assert n2 == n + 4 and cap2 >= max(n2, (3 * (n + 3)) // 2)  # at least x 1.5 and never less than the need
            img, lab = t.get_data()
            assert img.tobytes() == np.concatenate([pre_img, want["images"], more_img]).tobytes()
            assert lab.tobytes() == np.concatenate([pre_lab, want["labels"], more_lab]).tobytes()
            t.reserve(0)  # never below n
            assert t.count() == (n2, n2) and t.get_data()[0].tobytes() == img.tobytes()
        finally:
            t.close()
    finally:
        ctx.close()


# ---- 4. appends interleaved with training equal one set_data ----------------------------------------------------------------------
def test_interleaved_appends_equal_one_set_data():
    want = _label_view(3, 500)
    k = want["num_out"]
    a_img, a_lab = _random_set(3, 7, 9)
    rng = np.random.RandomState(10)
    first_steps = np.stack([rng.choice(7, 5, replace=False) for _ in range(2)]).astype(np.int32)
    later_steps = np.stack([rng.choice(7 + k, 5, replace=False) for _ in range(2)]).astype(np.int32)
    assert (later_steps >= 7).any()
    st0 = api.init_state(3, 3)
    ctx, cl = _context(CASES[3])
    try:
        online, whole = api.Trainer(ctx, max_batch=5), api.Trainer(ctx, max_batch=5)
        try:
            online.set_state(st0)
            online.append_data(a_img, a_lab)
            l1 = online.steps(first_steps)
            online.append_view(ctx, _rounds(cl, 6), 3, 500)
            l2 = online.steps(later_steps)
            online.append_data(a_img, a_lab, which=1)
            online.append_view(ctx, _rounds(cl, 6), 3, 500, which=1)

            all_img, all_lab = np.concatenate([a_img, want["images"]]), np.concatenate([a_lab, want["labels"]])
            whole.set_state(st0)
            whole.set_data(all_img, all_lab)
            w1 = whole.steps(first_steps)
            w2 = whole.steps(later_steps)
            whole.set_data(all_img, all_lab, which=1)

            assert l1.tobytes() == w1.tobytes() and l2.tobytes() == w2.tobytes()
            a, b = online.get_state(), whole.get_state()
            for key in api.TORCH_KEYS:
                assert a[key].tobytes() == b[key].tobytes(), key
            assert any(not np.array_equal(a[key], st0[key]) for key in a)
            la, ca = online.eval(n=7 + k, which=1)
            lb, cb = whole.eval(n=7 + k, which=1)
            assert la.tobytes() == lb.tobytes() and ca == cb
        finally:
            online.close()
            whole.close()
    finally:
        ctx.close()


# ---- 5. another context ------------------------------------------------------------------------------------------------------
def test_the_labelling_context_is_not_the_trainers():
    want = _label_view(15, 500)
    home = api.Context(api.default_params(15))
    ctx, cl = _context(CASES[15])
    try:
        t = api.Trainer(home)
        try:
            got = t.append_view(ctx, _rounds(cl, 6), 3, 500, want_all_labels=True)
            assert got["first"] == 0 and t.count()[0] == want["num_out"] == 6
            _assert_appended(got, want, t, 0)
        finally:
            t.close()
    finally:
        ctx.close()
        home.close()


# ---- 6. reorder --------------------------------------------------------------------------------------------------------------
def test_reorder():
    img, lab = _random_set(1, 12, 11)
    lab[:] = np.arange(12) % 2
    ctx = api.Context(api.default_params(1))
    try:
        t = api.Trainer(ctx)
        try:
            t.set_data(img, lab)

            def holds(order):
                gi, gl = t.get_data()
                assert gi.tobytes() == img[order].tobytes() and gl.tobytes() == lab[order].tobytes()

            now = np.arange(12)
            t.reorder(0, np.arange(12))  # the identity
            holds(now)
            t.reorder(0, np.arange(12)[::-1])  # a reversal
            now = now[::-1]
            holds(now)
            perm = np.random.RandomState(12).permutation(6)
            assert not np.array_equal(perm, np.arange(6))
            t.reorder(3, perm)  # a middle range: both neighbours stay
            now = np.concatenate([now[:3], now[3:9][perm], now[9:]])
            holds(now)
            t.reorder(5, np.zeros(0, np.int32))  # count 0
            t.reorder(12, np.zeros(0, np.int32))
            t.reorder(11, np.zeros(1, np.int32))  # count 1
            holds(now)
            for first, order in ((2, [0, 1, 1, 3]), (2, [0, 4, 2, 1]), (2, [0, -1, 2, 1]), (9, [0, 1, 2, 3]), (13, []), (-1, [0])):
                with pytest.raises(api.GpdHipError, match="error -1"):
                    t.reorder(first, np.array(order, np.int32))
                holds(now)
            with pytest.raises(api.GpdHipError, match="error -1"):
                t.reorder(0, np.arange(1), which=2)
            # the other entries' ranges
            for first, count in ((0, 13), (12, 1), (-1, 2), (5, -1)):
                with pytest.raises(api.GpdHipError, match="error -1"):
                    t.get_data(first, count)
            assert t.get_data(12, 0)[0].shape == (0, 60, 60, 1)
            two = lab.copy()
            two[3] = 2
            with pytest.raises(api.GpdHipError, match="label 2 of image 3"):
                t.append_data(img, two)
            assert t.count() == (12, 12)
            holds(now)
        finally:
            t.close()
    finally:
        ctx.close()


# ---- 7. past 4 GiB -----------------------------------------------------------------------------------------------------------
def test_a_pool_past_4_gib():
    far = 79535  # image 79536 straddles byte 2^32
    assert (far + 1) * IMAGE_BYTES_15 < 2 ** 32 < (far + 2) * IMAGE_BYTES_15
    probes, _ = _random_set(15, 3, 13)
    probe_lab = np.array([1, 0, 1], np.uint8)
    zeros, zero_lab = np.zeros((10000, 60, 60, 15), np.uint8), np.zeros(10000, np.uint8)
    ctx = api.Context(api.default_params(15))
    try:
        t = api.Trainer(ctx)
        try:
            t.set_state(api.init_state(15, 4))
            t.reserve(79540)
            assert t.count() == (0, 79540)
            t.append_data(probes, probe_lab)
            left = far - 3
            while left > 0:
                m = min(left, len(zeros))
                t.append_data(zeros[:m], zero_lab[:m])
                left -= m
            assert t.append_data(probes, probe_lab) == far
            assert t.count() == (far + 3, 79540)  # nothing was reallocated
            near_idx, far_idx = np.arange(3, dtype=np.int32), np.arange(far, far + 3, dtype=np.int32)
            # set_data keeps its limit, and refuses before it touches the set
            L = api.lib()
            rc = L.gpd_hip_train_set_data(t._h, 0, api._ptr(zeros), api._ptr(np.zeros(far + 3, np.uint8)), far + 3)
            assert rc == -3, rc
            assert t.count() == (far + 3, 79540)
            g_near, loss_near = t.gradients(near_idx)
            g_far, loss_far = t.gradients(far_idx)
            assert loss_near == loss_far and np.isfinite(loss_near)
            for key in api.TORCH_KEYS:
                assert g_near[key].tobytes() == g_far[key].tobytes(), key
            assert np.abs(g_near["conv1.weight"]).max() > 0
            assert t.eval(near_idx)[0].tobytes() == t.eval(far_idx)[0].tobytes()
            img, lab = t.get_data(far, 3)
            assert img.tobytes() == probes.tobytes() and lab.tobytes() == probe_lab.tobytes()
            img, lab = t.get_data(far - 2, 2)
            assert not img.any() and not lab.any()
            # a reorder across the boundary: the probes swap places on the device
            t.reorder(far, np.array([2, 1, 0], np.int32))
            img, lab = t.get_data(far, 3)
            assert img.tobytes() == probes[::-1].tobytes() and lab.tobytes() == probe_lab[::-1].tobytes()
        finally:
            t.close()
    finally:
        ctx.close()


# ---- 8. the whole loop -------------------------------------------------------------------------------------------------------
def test_the_whole_loop(tmp_path):
    from gpd_amd import hostlib
    from test_gpu_generate_data import CHANNELS, _composed, _data_set
    cfg, out_dir, clouds = _data_set(tmp_path)
    want = _composed(clouds)
    n_train, n_test = len(want[1]), len(want[3])
    assert n_train >= 5 and n_test > 0
    steps = np.stack([np.random.RandomState(14 + i).choice(n_train, 5, replace=False) for i in range(3)]).astype(np.int32)
    st0 = api.init_state(CHANNELS, 5)
    ctx = api.Context(api.default_params(CHANNELS))
    try:
        online, whole = api.Trainer(ctx, max_batch=5), api.Trainer(ctx, max_batch=5)
        try:
            assert hostlib.generate_data(cfg, online) == (n_train, n_test)
            assert (online.count(0)[0], online.count(1)[0]) == (n_train, n_test)
            for which in (0, 1):
                img, lab = online.get_data(which=which)
                assert img.tobytes() == want[2 * which].tobytes(), which
                assert lab.tobytes() == want[2 * which + 1].tobytes(), which
            assert not [f for f in os.listdir(str(out_dir)) if f.endswith(".npy")]
            whole.set_data(want[0], want[1], 0)
            whole.set_data(want[2], want[3], 1)
            results = []
            for t in (online, whole):
                t.set_state(st0)
                losses = t.steps(steps)
                logits, correct = t.eval(n=n_test, which=1)
                results.append((losses, t.get_state(), logits, correct))
            (la, sa, ga, ca), (lb, sb, gb, cb) = results
            assert la.tobytes() == lb.tobytes() and ga.tobytes() == gb.tobytes() and ca == cb
            for key in api.TORCH_KEYS:
                assert sa[key].tobytes() == sb[key].tobytes(), key
        finally:
            online.close()
            whole.close()
    finally:
        ctx.close()
    # the tool
    net = tmp_path / "net"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "gpd_amd.train", "--generate", str(cfg), "--epochs", "1", "--out", str(net)],
                         capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "training on %d images of %d channels, testing on %d" % (n_train, CHANNELS, n_test) in run.stdout
    assert (net / "network.cfg").exists() and len(os.listdir(str(net))) >= 9
    assert not [f for f in os.listdir(str(out_dir)) if f.endswith(".npy")]


# ---- 9. refusals before any work ---------------------------------------------------------------------------------------------
def test_refusals_before_any_work():
    pre_img, pre_lab = _random_set(15, 2, 15)
    cl = rcs.cloud()
    rounds = _rounds(cl, 6)
    three, _ = _context(CASES[3])
    ctx = api.Context(api.default_params(15))
    try:
        t = api.Trainer(ctx)
        try:
            t.append_data(pre_img, pre_lab)

            def refused(labeller, which, code):
                j = api.LabelViewJob()
                j.sample_indices, j.max_rounds, j.samples_per_round = api._ptr(rounds), rounds.shape[0], rounds.shape[1]
                j.min_positives, j.max_grasps_per_view = 3, 500
                assert api.lib().gpd_hip_train_append_view(t._h, which, labeller._h, C.byref(j)) == code
                assert (j.rounds_run, j.num_out, j.d2h_bytes) == (0, 0, 0)
                assert t.count() == (2, 2) and t.get_data()[0].tobytes() == pre_img.tobytes()

            refused(three, 0, -1)  # 3 channels against the trainer's 15
            assert "channels" in api.lib().gpd_hip_last_error().decode()
            ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
            for which in (-1, 2):
                refused(ctx, which, -1)
            refused(ctx, 0, -4)  # no ground truth uploaded
            assert "ground truth" in api.lib().gpd_hip_last_error().decode()
            for which in (-1, 2):
                for call in (lambda: t.reserve(4, which), lambda: t.count(which), lambda: t.append_data(pre_img, pre_lab, which),
                             lambda: t.get_data(0, 1, which)):
                    with pytest.raises(api.GpdHipError, match="error -1"):
                        call()
            assert t.count() == (2, 2)
        finally:
            t.close()
    finally:
        ctx.close()
        three.close()


# ---- 10. the shadow jitter of the labelling context ---------------------------------------------------------------------------
def test_append_view_images_with_the_shadow_jitter_of_the_labelling_context():
    """gpd_hip_set_shadow_jitter is state of the context that labels: a view appended from a context with the setting on lands
    in the pool with the images label_view returns on that context, one appended from a context with it off with the others —
    whichever context the trainer itself was made on.  One view of default_c15 (tests/entry_cases.py: its four rounds)."""
    import entry_cases as ec
    name, seed = "default_c15", ec.JITTER_SEED
    p, cl, _, _ = ec.inputs(name, api.default_params)
    gt, gn = ec.ground_truth(name)
    rounds = ec.view_rounds(name)
    shadow = [4, 9, 14]
    rest = [c for c in range(15) if c not in shadow]
    ctxs = []
    try:
        for on in (True, False):
            c = api.Context(p)
            ctxs.append(c)
            c.upload_ground_truth(gt, gn)
            c.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
            if on:
                c.set_shadow_jitter(True, seed)
        on_ctx, off_ctx = ctxs
        want_on = on_ctx.label_view(rounds, ec.MIN_POSITIVES, ec.MAX_GRASPS_PER_VIEW, want_all_labels=True)
        want_off = off_ctx.label_view(rounds, ec.MIN_POSITIVES, ec.MAX_GRASPS_PER_VIEW, want_all_labels=True)
        assert want_on["num_out"] == want_off["num_out"] == 6 and want_on["labels"].tobytes() == want_off["labels"].tobytes()
        assert want_on["images"][..., rest].tobytes() == want_off["images"][..., rest].tobytes()
        assert want_on["images"][..., shadow].tobytes() != want_off["images"][..., shadow].tobytes()
        for home in (on_ctx, off_ctx):
            t = api.Trainer(home)
            try:
                got = t.append_view(on_ctx, rounds, ec.MIN_POSITIVES, ec.MAX_GRASPS_PER_VIEW, want_all_labels=True)
                _assert_appended(got, want_on, t, 0)
                got = t.append_view(off_ctx, rounds, ec.MIN_POSITIVES, ec.MAX_GRASPS_PER_VIEW, want_all_labels=True)
                assert got["first"] == want_on["num_out"]
                _assert_appended(got, want_off, t, 0)
                img, _ = t.get_data(0, 2 * want_on["num_out"])
                assert img[:6].tobytes() == want_on["images"].tobytes() != img[6:].tobytes()
            finally:
                t.close()
    finally:
        for c in ctxs:
            c.close()
