"""The shape-general LeNet route on the device (gpd_hip_set_lenet_net): other layer widths and NetCCFFF of the reference's
pytorch/network.py, defined bit for bit by the k-ascending f32 fmaf chains of lenet_net_ref.py (built from
oracle.conv_generic, none of the code under test).

  * scores and all five activation tensors equal the chain network at every batch size, for shapes under one tile (A), one past
    a tile edge (B), wide (C), stock (D) and at every upper limit (E); A and B also without the conv ReLUs and with the conv
    weights negated (clamps elsewhere) — a kernel that reorders a chain, pads inside it or reads past a width fails these;
  * the stock shape agrees with GPD_LENET_F32_CHAIN (another kernel set, the same definition), and gpd_hip_set_lenet_weights
    returns the context to the stock route;
  * an image scores the same in whichever chunk of a long batch it stands;
  * the fused entries and the host layer score with the installed network.
"""
import os
import subprocess

import numpy as np
import pytest

import lenet_net_ref as R
import lenet_torch_ref as ltr
from gpd_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG = ((0, "pool1"), (1, "pool2"), (2, "fc1"), (3, "fc2"), (4, "logits"))


def _ctx(C):
    from gpd_amd import api
    return api.Context(api.default_params(C))


def _check_against_chain(ctx, name, want, n, label, imgs=None):
    """Scores, then the debug tensors in layer order: the first tensor that differs is the assertion that fails.  imgs: other
    images than R.images(name) (at most 35: image i of the batch is image i % 35 of them, as want is indexed)"""
    idx = np.arange(n) % ltr.N_IMAGES
    sc = ctx.score(R.images(name, n) if imgs is None else imgs[idx % len(imgs)])
    bad = np.flatnonzero(sc != want["score"][idx])
    print("%s n = %d: %d scores differ from the chain%s" % (label, n, len(bad), "" if not len(bad) else
                                                             ", max |diff| = %.3g" % float(np.abs(sc - want["score"][idx]).max())))
    for which, key in DEBUG:
        if want[key] is None:
            continue
        got = ctx.lenet_net_debug(which, n)
        diff = got != want[key][idx]
        if diff.any():
            print("%s n = %d %s: %d of %d values differ, max |diff| = %.3g" % (label, n, key, int(diff.sum()), diff.size,
                                                                               float(np.abs(got - want[key][idx]).max())))
        assert np.array_equal(got, want[key][idx]), (label, n, key)
    assert np.array_equal(sc, want["score"][idx]), (label, n, bad[:5])
    return sc


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_scores_and_activations_are_the_chain_bit_for_bit(name):
    from gpd_amd import api
    C, F1, F2, H1, H2 = R.SHAPES[name]
    runs = [(False, True)] + ([(False, False), (True, True)] if name in "AB" else [])  # (negated, conv_relu)
    ctx = _ctx(C)
    try:
        for negated, relu in runs:
            shape = ctx.set_lenet_net(R.state(name, negated), R.INPUT_SCALE, conv_relu=relu)
            assert shape.as_tuple() == R.SHAPES[name]
            info = ctx.lenet_net_info()
            assert 1 <= info["chunk_images"] <= 65536 and info["chunk_images"] * info["scratch_bytes_per_image"] <= 6 << 30
            assert info["lds_bytes"] <= 160 * 1024
            assert info["macs_per_image"] == F1 * 3136 * C * 25 + F2 * 576 * F1 * 25 + F2 * 144 * H1 + H1 * (H2 or 2) + H2 * 2
            want = R.chain(name, negated, relu)
            if relu:  # clamped values are exactly zero, and there are some
                assert want["pool1"].min() == 0 and want["pool2"].min() == 0 and (want["pool1"] == 0).mean() > 0.02
            else:
                assert want["pool1"].min() < 0 and want["pool2"].min() < 0
            for n in R.BATCHES[name]:
                _check_against_chain(ctx, name, want, n, "%s negated = %d relu = %d" % (name, negated, relu))
            if not H2:
                with pytest.raises(api.GpdHipError):
                    ctx.lenet_net_debug(3, 1)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["B", "D"])
def test_blank_image_areas_change_no_bit(name, oracle_mod):
    """Grasp images are mostly blank in places, and conv1 passes over k steps whose inputs are all zero: images with blank
    channels, blank rows and a blank half, and an image of zeros, against the chain network (which multiplies every zero)"""
    C = R.SHAPES[name][0]
    img = R.images(name, 5).copy()
    img[0, :, :, C // 2:] = 0      # the later channels (the last one of C = 1: the whole image)
    img[1, 10:50] = 0              # a band of rows in every channel
    img[2, :, 30:] = 0             # the right half
    img[3] = 0
    img[3, 17, 43, 0] = 200        # one pixel
    img[4] = 0
    want = R.chain_batch(oracle_mod, R.SHAPES[name], R.route_arrays(name)[1], img)
    ctx = _ctx(C)
    try:
        ctx.set_lenet_net(R.state(name))
        for n in (5, 1):
            sc = ctx.score(img[:n])
            assert np.array_equal(ctx.lenet_net_debug(0, n), want["pool1"][:n])
            assert np.array_equal(ctx.lenet_net_debug(4, n), want["logits"][:n])
            assert np.array_equal(sc, want["score"][:n])
    finally:
        ctx.close()


def test_stock_shape_agrees_with_the_chain_mode_and_weights_return_to_the_stock_route():
    from gpd_amd import api
    C = R.SHAPES["D"][0]
    st = R.state("D")
    img = R.images("D", 35)
    ctx = _ctx(C)
    try:
        with pytest.raises(api.GpdHipError):
            ctx.lenet_net_info()  # nothing installed
        ctx.set_lenet_mode(api.LENET_F32_CHAIN)
        ctx.set_lenet_torch(st)
        stock_chain = ctx.score(img)
        ctx.set_lenet_mode(api.LENET_SPLIT)
        stock_split = ctx.score(img)
        out = np.zeros(2, np.float32)
        assert api.lib().gpd_hip_lenet_net_debug(ctx._h, 4, 1, out.ctypes.data) == -1  # the stock route ran
        ctx.set_lenet_net(st)
        general = ctx.score(img)
        assert np.array_equal(general, stock_chain)  # two kernel sets, one definition
        assert np.array_equal(general, R.chain("D")["score"])
        assert np.array_equal(ctx.lenet_net_debug(4, 35), R.chain("D")["logits"])
        ctx.set_lenet_weights(api.lenet_from_torch(st, C))
        assert np.array_equal(ctx.score(img), stock_split)  # the mode the context was left in, bit for bit as before
        assert api.lib().gpd_hip_lenet_net_debug(ctx._h, 4, 1, out.ctypes.data) == -1
        with pytest.raises(api.GpdHipError, match="general route"):
            ctx.lenet_net_debug(4, 1)
        ctx.set_lenet_mode(api.LENET_F32_CHAIN)
        assert np.array_equal(ctx.score(img), stock_chain)
        # refusals: another channel count, a non-finite weight
        with pytest.raises(api.GpdHipError, match="image_num_channels"):
            ctx.set_lenet_net(R.state("A"))
        bad = dict(st, **{"fc1.bias": np.full(500, np.inf, np.float32)})
        with pytest.raises(api.GpdHipError, match="not finite"):
            ctx.set_lenet_net(bad)
        assert np.array_equal(ctx.score(img), stock_chain)  # a refused network leaves the installed one alone
    finally:
        ctx.close()


def test_scores_do_not_depend_on_the_chunk():
    """Shape E, one channel: one chunk and 35 images more, the 35 test images repeated (about 83 MB)"""
    name = "E"
    ctx = _ctx(R.SHAPES[name][0])
    try:
        ctx.set_lenet_net(R.state(name))
        chunk = ctx.lenet_net_info()["chunk_images"]
        assert chunk < 65536  # the 6 GiB bound, not the image bound, cuts this shape
        n = chunk + 35
        sc = ctx.score(R.images(name, n))
        first = sc[:35]
        want = R.chain(name, n=35)["score"]
        print("E: %d images in chunks of %d; %d of the first 35 differ from the chain" % (n, chunk, int((first != want).sum())))
        assert np.array_equal(first, want)
        assert np.array_equal(sc, first[np.arange(n) % 35])
    finally:
        ctx.close()


def test_fused_entries_score_with_the_installed_network(oracle_mod):
    from gpd_amd import api
    name = "A"
    C = R.SHAPES[name][0]
    cloud = synth.make_cloud(5, 2000)
    si = synth.sample_indices(cloud, 30)
    ctx = _ctx(C)
    try:
        ctx.set_lenet_net(R.state(name))
        ctx.upload_cloud(cloud["xyz"], cloud["normals"], cloud["cam_source"], cloud["view_points"])
        dh, n_cand = ctx.detect(si)
        dh = dh.copy()
        assert ctx.lenet_net_debug(4, 1).shape == (1, 2)  # the fused call took the general route
        img, cand = ctx.images(dh)
        assert len(cand) == n_cand >= 20
        want = ctx.score(img)
        assert np.array_equal(dh.reshape(-1)[cand]["score"], want)
        (bh, _, bnc, _), = ctx.detect_batch([cloud], [si], 0)
        assert bnc == len(cand) and np.array_equal(bh["score"], want)
        scored, gs, gcand, _ = ctx.score_given(dh)
        assert np.array_equal(gcand, cand) and np.array_equal(gs, want) and np.array_equal(scored.reshape(-1)[cand]["score"], want)
        ref = R.chain_batch(oracle_mod, R.SHAPES[name], R.route_arrays(name)[1], img)["score"]
        assert np.array_equal(want, ref)
        for mode in (api.LENET_F32_CHAIN, api.LENET_SPLIT):  # accepted and ignored
            ctx.set_lenet_mode(mode)
            assert ctx.score(img).tobytes() == want.tobytes()
            assert np.array_equal(ctx.detect(si)[0].reshape(-1)[cand]["score"], want)
        stock = _ctx(C)
        try:  # the stock network on the same images gives other scores
            stock.set_lenet_torch(ltr.state(C))
            assert np.abs(stock.score(img) - want).max() > 1e-3
        finally:
            stock.close()
    finally:
        ctx.close()


def test_detect_grasps_on_an_exported_netccfff_directory(tmp_path):
    import torch
    from gpd_amd import api, torch_export
    from test_host_cli import CLI, _subsample_indices, _write_case
    name = "A"
    C, S, K = R.SHAPES[name][0], 30, 10
    cl = synth.make_cloud(5, 2000)
    st = R.state(name)
    cfg, pcd = _write_case(tmp_path, cl, ltr.eigen_weights(C), S, K, channels=C)
    params = tmp_path / "params"
    for f in os.listdir(str(params)):  # the Eigen-layout files _write_case wrote: this directory is a torch one
        os.remove(str(params / f))
    model = tmp_path / "model.pwf"
    torch.save({k: torch.from_numpy(v.copy()) for k, v in st.items()}, str(model))
    assert torch_export.main([str(model), str(params)]) == 0
    out = subprocess.run([CLI, str(cfg), str(pcd)], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = np.array([float(l.split()[1]) for l in out.stdout.splitlines() if l.startswith("GRASP ")], np.float32)
    ctx = _ctx(C)
    try:
        ctx.set_lenet_net(st)
        ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
        sel, _, n_cand = ctx.detect_select(_subsample_indices(len(cl["xyz"]), S), K)
        assert len(sel) == K and n_cand > K
        assert np.array_equal(got, sel["score"])
    finally:
        ctx.close()
    # a directory whose fc2.weight.bin has the stock size is refused
    np.zeros(1000, "<f4").tofile(str(params / "fc2.weight.bin"))
    out = subprocess.run([CLI, str(cfg), str(pcd)], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert "missing or have unexpected sizes" in out.stdout
    assert not [l for l in out.stdout.splitlines() if l.startswith("GRASP ")]
