"""gpd_hip_set_lenet_conv_relu on the device: the network of the reference's PyTorch scripts (pytorch/network.py::Net — a ReLU
after conv1 and conv2, inputs / 256, channel-major flatten, nn.Linear layouts) through both scoring modes, the fused entries
and the host layer.  References and inputs: lenet_torch_ref.py (computed once, shared).

  * GPD_LENET_F32_CHAIN: scores and pool1 bit-identical to the k-ascending f32 fmaf chains built from oracle.conv_generic;
  * GPD_LENET_SPLIT: pool1 and the flattened pool2 non-negative and, per element, within 4 x the error the test's own torch
    float32 forward makes against float64 on the same tensor (one f32 summation order is a sample of f32 error, not a bound:
    hence the factor); scores within 1e-4 of float64 (the project's score contract);
  * both with a second weight set (conv weights and biases negated), so that every one of the 20 + 50 channels is clamped
    somewhere — conv2's two epilogues (filters 0..47, filters 48 and 49) included;
  * batch sizes 1, 2, 3 and 35: the persistent conv kernels take two images per workgroup and up, ip2 works in blocks of 32
    images, ip1's X operand is blocked by 16.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import lenet_ref
import lenet_torch_ref as ltr
from gpd_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ctx(C, mode):
    from gpd_amd import api
    ctx = api.Context(api.default_params(C))
    ctx.set_lenet_mode(mode)
    return ctx


@pytest.mark.parametrize("C", [15, 12, 3, 1])
def test_chain_mode_is_the_fmaf_chain_network_bit_for_bit(C):
    from gpd_amd import api
    assert ltr.every_channel_clamps(C)  # a condition on the inputs (float64 truth): change the seed, not the condition
    img = ltr.images(C)
    ctx = _ctx(C, api.LENET_F32_CHAIN)
    try:
        for negated in (False, True):
            ctx.set_lenet_torch(ltr.state(C, negated))
            want_p1, want_sc = ltr.chain(C, negated)
            for n in ltr.BATCHES:
                sc = ctx.score(img[:n])
                p1 = ltr.chain_pool1_planes(ctx.lenet_debug(0, n), n)
                bad = np.flatnonzero(sc != want_sc[:n])
                print("C = %d, negated = %d, n = %d: %d scores differ, max |pool1 - chain| = %.3g"
                      % (C, negated, n, len(bad), float(np.abs(p1 - want_p1[:n]).max())))
                assert np.array_equal(p1, want_p1[:n]), (negated, n)
                assert np.array_equal(sc, want_sc[:n]), (negated, n, bad[:5])
                assert p1.min() >= 0
    finally:
        ctx.close()


@pytest.mark.parametrize("C", [15, 12, 3, 1])
def test_split_mode_against_float64(C):
    from gpd_amd import api
    assert ltr.every_channel_clamps(C)
    img = ltr.images(C)
    ctx = _ctx(C, api.LENET_SPLIT)
    try:
        for negated in (False, True):
            ctx.set_lenet_torch(ltr.state(C, negated))
            t64, t32 = ltr.truth(C, negated), ltr.truth(C, negated, "float32")
            for n in ltr.BATCHES:
                sc = ctx.score(img[:n])
                p1 = np.transpose(ctx.lenet_debug(0, n).reshape(n, 28, 28, 20), (0, 3, 1, 2))     # -> [n][filter][row][column]
                xs = ctx.lenet_debug(1, n)
                flat = lenet_ref.bf16_to_f64(xs[0]) + lenet_ref.bf16_to_f64(xs[1]) + lenet_ref.bf16_to_f64(xs[2])
                p2 = np.transpose(flat.reshape(n, 144, 50), (0, 2, 1)).reshape(n, 50, 12, 12)       # flat index = pixel * 50 + filter
                assert p1.min() >= 0 and p2.min() >= 0, (negated, n)
                for name, got in (("pool1", p1), ("pool2", p2)):
                    yard = float(np.abs(t32[name][:n].astype(np.float64) - t64[name][:n]).max())
                    err = float(np.abs(got.astype(np.float64) - t64[name][:n]).max())
                    print("C = %d, negated = %d, n = %d, %s: max |device - f64| = %.3g, torch f32's = %.3g" % (C, negated, n, name, err, yard))
                    assert err <= 4 * yard, (name, negated, n, err, yard)
                # the clamp took place where the truth says so (a value the truth puts clearly below zero is zero on the device)
                assert (p1[t64["pre1"][:n] < -1e-3] == 0).all() and (p2[t64["pre2"][:n] < -1e-3] == 0).all()
                err = float(np.abs(sc - t64["score"][:n]).max())
                print("C = %d, negated = %d, n = %d: max |score - f64| = %.3g" % (C, negated, n, err))
                assert err <= 1e-4, (negated, n, err)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_flag_is_context_state(mode):
    """Off again gives back, bit for bit, the scores taken before it was turned on; weights set after the flag keep it; and a
    value other than 0 / 1 is refused."""
    from gpd_amd import api
    C = 3
    img = ltr.images(C)
    w = api.lenet_from_torch(ltr.state(C), C)
    ctx = _ctx(C, mode)
    try:
        ctx.set_lenet_weights(w)
        before = ctx.score(img)
        ctx.set_lenet_conv_relu(True)
        on = ctx.score(img)
        assert np.abs(on - before).max() > 1e-3  # another network
        ctx.set_lenet_weights(w)                 # ... which new weights do not switch off
        assert np.array_equal(ctx.score(img), on)
        ctx.set_lenet_conv_relu(False)
        assert np.array_equal(ctx.score(img), before)
        assert api.lib().gpd_hip_set_lenet_conv_relu(ctx._h, 2) == -1
        assert np.array_equal(ctx.score(img), before)
    finally:
        ctx.close()
    # the flag before any weights
    ctx = _ctx(C, mode)
    try:
        ctx.set_lenet_conv_relu(True)
        ctx.set_lenet_weights(w)
        assert np.array_equal(ctx.score(img), on)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_fused_entries_score_with_the_flag(mode, oracle_mod):
    """gpd_hip_detect and one job through gpd_hip_detect_batch with the flag on: every valid hand carries the score
    gpd_hip_score gives the same candidate's image under the same flag; in chain mode that is the fmaf-chain network's."""
    from gpd_amd import api
    C = 15
    cloud = synth.make_cloud(5, 2000)
    si = synth.sample_indices(cloud, 30)
    ctx = _ctx(C, mode)
    try:
        ctx.set_lenet_torch(ltr.state(C))
        ctx.upload_cloud(cloud["xyz"], cloud["normals"], cloud["cam_source"], cloud["view_points"])
        dh, n_cand = ctx.detect(si)
        dh = dh.copy()
        # the candidates of the fused call (its valid hands: the workspace filter has run) through the stepwise entries
        img, cand = ctx.images(dh)
        assert len(cand) == n_cand >= 20
        want = ctx.score(img)
        assert np.array_equal(dh.reshape(-1)[cand]["score"], want)
        off = api.Context(api.default_params(C))
        try:  # the same weights without the flag give other scores: the fused path did not simply ignore it
            off.set_lenet_mode(mode)
            off.set_lenet_weights(api.lenet_from_torch(ltr.state(C), C))
            assert np.abs(off.score(img) - want).max() > 1e-3
        finally:
            off.close()
        (bh, _, bnc, _), = ctx.detect_batch([cloud], [si], 0)
        assert bnc == len(cand) and np.array_equal(bh["score"], want)
        if mode == api.LENET_F32_CHAIN:
            w = api.lenet_from_torch(ltr.state(C), C)
            ref = np.array([o[2] for o in ltr.chain_batch(oracle_mod, w, img)], np.float32)
            assert np.array_equal(want, ref)
    finally:
        ctx.close()


def test_detect_grasps_on_an_exported_directory(tmp_path):
    """The host layer on a directory written by gpd_amd.torch_export: the scores detect_grasps prints are the Python path's
    (Context.set_lenet_torch on the same state dict); a network.cfg that names another layout is refused."""
    import torch
    from gpd_amd import api, torch_export
    from test_host_cli import CLI, _subsample_indices, _write_case
    C, S, K = 15, 30, 10
    cl = synth.make_cloud(5, 2000)
    st = ltr.state(C)
    cfg, pcd = _write_case(tmp_path, cl, ltr.eigen_weights(C), S, K)
    params = tmp_path / "params"
    for f in os.listdir(str(params)):  # the Eigen-layout files _write_case wrote: this directory is a torch one
        os.remove(str(params / f))
    model = tmp_path / "model.pwf"
    torch.save({k: torch.from_numpy(v.copy()) for k, v in st.items()}, str(model))
    assert torch_export.main([str(model), str(params)]) == 0
    out = subprocess.run([CLI, str(cfg), str(pcd)], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = np.array([float(l.split()[1]) for l in out.stdout.splitlines() if l.startswith("GRASP ")], np.float32)
    ctx = api.Context(api.default_params(C))
    try:
        ctx.set_lenet_torch(st)
        ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
        si = _subsample_indices(len(cl["xyz"]), S)
        sel, _, n_cand = ctx.detect_select(si, K)
        assert len(sel) == K and n_cand > K
        assert np.array_equal(got, sel["score"])
        ctx.set_lenet_conv_relu(False)  # the CLI did set the flag: without it the same weights give other scores
        assert not np.array_equal(ctx.detect_select(si, K)[0]["score"], got)
    finally:
        ctx.close()
    (params / "network.cfg").write_text("layout = onnx\nconv_relu = 1\ninput_scale = 0.00390625\n")
    out = subprocess.run([CLI, str(cfg), str(pcd)], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert "unknown layout 'onnx'" in out.stdout and "ERROR" in out.stdout
    assert not [l for l in out.stdout.splitlines() if l.startswith("GRASP ")]
    # ... and so is a torch directory whose files have the wrong sizes
    assert torch_export.main([str(model), str(params)]) == 0
    np.zeros(7, "<f4").tofile(str(params / "fc1.weight.bin"))
    out = subprocess.run([CLI, str(cfg), str(pcd)], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert "missing or have unexpected sizes" in out.stdout
    assert not [l for l in out.stdout.splitlines() if l.startswith("GRASP ")]
