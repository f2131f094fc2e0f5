"""GPD_LENET_NET_SPLIT (gpd_hip_set_lenet_net_mode): the shape-general LeNet route on the bf16 matrix pipe, held against the
arithmetic users have today — the f32 chain, computed on the CPU by oracle.conv_generic with none of the code under test.

Per layer, on the device's OWN input (the images for conv1, the previous debug tensor otherwise): ref64 is the layer in float64,
e_chain = max |chain32(layer) - ref64| on the same input, e_split = max |device - ref64|, and
    e_split <= 4 e_chain + 2 spacing(float32(max |ref64|)).
A split that omits one second-order product (h*l or m*m) lands at 2.2 - 11.8 times that allowance for K <= 500 and inside it from
K ~ 7200 on, so every kernel is also checked at a small K: conv1 at K = 25 (B, I), 75 (A, G), 300 (F), 375 (D, H); conv2 at
K = 150 (A), 175 (F), 225 (G); the dense kernel at fc2 K = 120 (A), 130 (F) and 1 (G) and at fc1 K = 144 (G, I).  The logits are the
chain's, bit for bit, on the device's last hidden tensor.  End to end the same allowance holds against the float64 network with
the CPU chain network as the yardstick.  Then: determinism and batch independence, magnitudes inside the stated domain, the
mode's plumbing, and every composed entry."""
import os
import subprocess

import numpy as np
import pytest

import lenet_net_ref as R
import lenet_torch_ref as ltr
from gpd_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG = ((0, "pool1"), (1, "pool2"), (2, "fc1"), (3, "fc2"), (4, "logits"))
CHAIN, SPLIT = api.LENET_NET_CHAIN, api.LENET_NET_SPLIT


def _ctx(C):
    return api.Context(api.default_params(C))


def _split_ctx(name="A", **kw):
    ctx = _ctx(R.ALL_SHAPES[name][0])
    ctx.set_lenet_net(R.state(name), R.INPUT_SCALE, net_mode=SPLIT, **kw)
    return ctx


def _tensors(ctx, shape, n):
    return {key: ctx.lenet_net_debug(which, n) for which, key in DEBUG if which != 3 or shape[4]}


def _allowance(e_chain, ref64):
    return 4.0 * e_chain + 2.0 * float(np.spacing(np.float32(np.abs(ref64).max())))


def _conv_layer(oracle, x, w, b, relu):
    """x [n, C, H, H] f32 (exact values), w [F, C, 5, 5] f32, b [F] -> (ref64, chain32), each [n, F, P, P]: 5x5 valid
    convolution, 2x2 max-pool on the sums, + bias, the optional ReLU"""
    import torch
    import torch.nn.functional as F
    with torch.no_grad():
        y = F.max_pool2d(F.conv2d(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(w.astype(np.float64))), 2)
        y = y + torch.from_numpy(b.astype(np.float64)).reshape(1, -1, 1, 1)
        ref = (F.relu(y) if relu else y).numpy()
    chain = np.stack([R._pool(oracle.conv_generic(np.ascontiguousarray(xi, np.float32), w, b)) for xi in x])
    return ref, (np.maximum(chain, np.float32(0)) if relu else chain)


def _dense_layer(oracle, x, w_ku, b):
    """x [n, K] f32, w_ku [K, U], b [U] -> (ref64, chain32) of ReLU(x w + b)"""
    ref = np.maximum(x.astype(np.float64) @ w_ku.astype(np.float64) + b.astype(np.float64), 0.0)
    chain = np.stack([np.maximum(R._dense_chain(oracle, xi, w_ku, b), np.float32(0)) for xi in x])
    return ref, chain


def _check_layers(oracle, shape, arrs, relu, img, dev, label):
    """Every layer of the device's tensors `dev` on its own input; prints each figure before it asserts -> {layer: (e_split, e_chain)}"""
    C, F1, F2, H1, H2 = shape
    n = len(img)
    x0 = np.ascontiguousarray(np.transpose(img, (0, 3, 1, 2))).astype(np.float32)
    flat = np.ascontiguousarray(dev["pool2"].reshape(n, F2, 144).transpose(0, 2, 1)).reshape(n, -1)  # k = pixel * F2 + channel
    layers = [("conv1", dev["pool1"], lambda: _conv_layer(oracle, x0, arrs[0].reshape(F1, C, 5, 5), arrs[1], relu)),
              ("conv2", dev["pool2"], lambda: _conv_layer(oracle, dev["pool1"], arrs[2].reshape(F2, F1, 5, 5), arrs[3], relu)),
              ("fc1", dev["fc1"], lambda: _dense_layer(oracle, flat, arrs[4].reshape(F2 * 144, H1), arrs[5]))]
    if H2:
        layers.append(("fc2", dev["fc2"], lambda: _dense_layer(oracle, dev["fc1"], arrs[6].reshape(H1, H2), arrs[7])))
    out, failed = {}, []
    for layer, got, refs in layers:
        assert np.isfinite(got).all(), (label, layer)
        ref64, chain32 = refs()
        e_chain = float(np.abs(chain32.astype(np.float64) - ref64).max())
        e_split = float(np.abs(got.astype(np.float64) - ref64).max())
        allow = _allowance(e_chain, ref64)
        print("%s %s: e_split = %.3g, e_chain = %.3g, allowance = %.3g (e_split / allowance = %.2f)" % (label, layer, e_split, e_chain, allow,
                                                                                                         e_split / allow))
        out[layer] = (e_split, e_chain)
        if not e_split <= allow:
            failed.append((layer, e_split, e_chain, allow))
        if relu or layer.startswith("fc"):  # clamped values are exactly +0
            zeros = got == 0
            assert got.min() >= 0 and not np.signbit(got[zeros]).any(), (label, layer)
            assert ((ref64 == 0) <= ((got == 0) | (np.abs(got) <= allow))).all(), (label, layer)
    hid, lw, lb = (dev["fc2"], arrs[8].reshape(H2, 2), arrs[9]) if H2 else (dev["fc1"], arrs[6].reshape(H1, 2), arrs[7])
    want = np.stack([R._dense_chain(oracle, h, lw, lb) for h in hid])
    assert np.array_equal(dev["logits"], want), (label, "logits")
    assert not failed, (label, failed)
    return out


# (shape, negated, conv_relu, images)
LAYER_RUNS = [(name, False, True, 6) for name in "ABDFGHI"] + [("A", False, False, 6), ("B", False, False, 6), ("A", True, True, 6), ("B", True, True, 6),
                                                               ("E", False, True, 3)]


@pytest.mark.parametrize("name,negated,relu,n", LAYER_RUNS, ids=["%s%s%s" % (r[0], "-negated" if r[1] else "", "" if r[2] else "-norelu") for r in LAYER_RUNS])
def test_every_layer_and_the_score_are_within_four_chain_errors(name, negated, relu, n, oracle_mod):
    shape = R.ALL_SHAPES[name]
    arrs = R.numpy_route_arrays(R.state(name, negated))
    img = R.images(name, n)
    label = "%s negated = %d relu = %d" % (name, negated, relu)
    ctx = _ctx(shape[0])
    try:
        ctx.set_lenet_net(R.state(name, negated), R.INPUT_SCALE, conv_relu=relu, net_mode=SPLIT)
        info = ctx.lenet_net_info()
        C, F1, F2, H1, H2 = shape
        assert info["lds_bytes"] <= 160 * 1024 and 1 <= info["chunk_images"] <= 65536
        assert info["chunk_images"] * info["scratch_bytes_per_image"] <= 6 << 30
        assert info["macs_per_image"] == F1 * 3136 * C * 25 + F2 * 576 * F1 * 25 + F2 * 144 * H1 + H1 * (H2 or 2) + H2 * 2
        score = ctx.score(img)
        dev = _tensors(ctx, shape, n)
    finally:
        ctx.close()
    assert np.array_equal(score, dev["logits"][:, 1] - dev["logits"][:, 0])
    _check_layers(oracle_mod, shape, arrs, relu, img, dev, label)
    if relu:
        assert (dev["pool1"] == 0).any() and (dev["pool2"] == 0).any()
    # end to end: the float64 network is the truth, the CPU chain network the yardstick
    import torch
    truth = R.forward(R.state(name, negated), img, torch.float64, relu)["score"]
    chain = R.chain(name, negated, relu)["score"][:n]
    e_chain, e_split = float(np.abs(chain - truth).max()), float(np.abs(score - truth).max())
    allow = _allowance(e_chain, truth)
    print("%s score: e_split = %.3g, e_chain = %.3g, allowance = %.3g" % (label, e_split, e_chain, allow))
    assert e_split <= allow, (label, e_split, e_chain)


BATCHES = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)


def test_scores_and_tensors_do_not_depend_on_the_batch_and_repeat():
    name = "F"
    shape = R.ALL_SHAPES[name]
    ctx = _split_ctx(name)
    try:
        base = ctx.score(R.images(name, 35))
        want = _tensors(ctx, shape, 35)
        assert len(np.unique(base)) >= 30
        for n in BATCHES:
            img = R.images(name, n)
            idx = np.arange(n) % 35
            sc = ctx.score(img)
            assert np.array_equal(sc, base[idx]), n
            got = _tensors(ctx, shape, n)
            for key in want:
                assert np.array_equal(got[key], want[key][idx]), (n, key)
            assert ctx.score(img).tobytes() == sc.tobytes(), n
    finally:
        ctx.close()


def test_scores_do_not_depend_on_the_chunk():
    """Shape I (the smallest scratch: the chunk is the 65536-image bound): one chunk and 35 images more"""
    name = "I"
    ctx = _split_ctx(name)
    try:
        first = ctx.score(R.images(name, 35))
        chunk = ctx.lenet_net_info()["chunk_images"]
        assert chunk == 65536
        n = chunk + 35
        sc = ctx.score(R.images(name, n))
        assert np.array_equal(sc[:35], first)
        assert np.array_equal(sc, first[np.arange(n) % 35])
    finally:
        ctx.close()


def _scaled_state():
    """A seeded F inside the domain of the split mode (no operand below 2^-100 but zeros): one conv1 filter times 2^60, undone by
    2^-60 on that input channel of conv2; one fc1 unit times 2^30, undone in fc2; one row of each layer with weights spanning
    e^-12 .. 1; one all-zero row"""
    shape = R.ALL_SHAPES["F"]
    C, F1, F2, H1, H2 = shape
    rng = np.random.RandomState(4242)
    st = {k: v.copy() for k, v in R.make_state(shape, 5).items()}
    f32 = np.float32
    c1 = st["conv1.weight"].reshape(F1, C * 25)
    c1[1] *= f32(2.0 ** 60)
    st["conv1.bias"][1] *= f32(2.0 ** 60)
    st["conv2.weight"][:, 1] *= f32(2.0 ** -60)
    st["fc1.weight"][3] *= f32(2.0 ** 30)
    st["fc1.bias"][3] *= f32(2.0 ** 30)
    st["fc2.weight"][:, 3] *= f32(2.0 ** -30)
    for key, row in (("conv1.weight", 2), ("conv2.weight", 2), ("fc1.weight", 2), ("fc2.weight", 2)):
        w = st[key].reshape(st[key].shape[0], -1)
        w[row] *= np.exp(rng.uniform(-12, 0, w.shape[1])).astype(f32)
    for key, row in (("conv1.weight", 3), ("conv2.weight", 4), ("fc1.weight", 5), ("fc2.weight", 6)):
        st[key][row] = 0
    for v in st.values():
        a = np.abs(v[v != 0])
        assert np.isfinite(v).all() and a.min() >= 2.0 ** -100
    return st


def test_magnitudes_inside_the_domain(oracle_mod):
    name = "F"
    shape = R.ALL_SHAPES[name]
    st = _scaled_state()
    img = R.hostile_images(name)  # twelve seeded images, one of 255s, one of zeros, one without a zero pixel
    assert len(img) == 15
    ctx = _ctx(shape[0])
    try:
        ctx.set_lenet_net(st, R.INPUT_SCALE, net_mode=SPLIT)
        score = ctx.score(img)
        dev = _tensors(ctx, shape, len(img))
    finally:
        ctx.close()
    assert np.isfinite(score).all() and dev["pool1"].max() > 2.0 ** 50
    for key, v in dev.items():  # the activations stay inside the domain too
        nz = np.abs(v[v != 0])
        assert nz.size and nz.min() >= 2.0 ** -100, key
    _check_layers(oracle_mod, shape, R.numpy_route_arrays(st), True, img, dev, "F scaled")


def test_mode_plumbing():
    name = "A"
    shape = R.ALL_SHAPES[name]
    C, F1, F2, H1, H2 = shape
    img = R.images(name, 35)
    want_chain = R.chain(name)["score"]
    ctx = _ctx(C)
    try:
        ctx.set_lenet_net(R.state(name))
        chain_info = ctx.lenet_net_info()
        assert np.array_equal(ctx.score(img), want_chain)  # the default is the chain
        ctx.set_lenet_net_mode(SPLIT)  # after the install ...
        with pytest.raises(api.GpdHipError, match="general route"):
            ctx.lenet_net_debug(4, 1)  # the chain's scratch is gone, nothing ran in the split one
        split = ctx.score(img)
        assert (split != want_chain).any() and np.abs(split - want_chain).max() < 1e-4
        info = ctx.lenet_net_info()
        assert info["lds_bytes"] <= 160 * 1024 and info["chunk_images"] * info["scratch_bytes_per_image"] <= 6 << 30
        assert info["macs_per_image"] == chain_info["macs_per_image"]
        assert info["scratch_bytes_per_image"] != chain_info["scratch_bytes_per_image"]
        for mode in (api.LENET_F32_CHAIN, api.LENET_SPLIT):  # gpd_hip_set_lenet_mode: accepted and ignored
            ctx.set_lenet_mode(mode)
            assert ctx.score(img).tobytes() == split.tobytes()
        ctx.set_lenet_net_mode(CHAIN)
        assert ctx.lenet_net_info() == chain_info
        for mode in (api.LENET_F32_CHAIN, api.LENET_SPLIT):
            ctx.set_lenet_mode(mode)
            assert np.array_equal(ctx.score(img), want_chain)
        with pytest.raises(api.GpdHipError, match="gpd_hip_set_lenet_net_mode: bad argument"):
            ctx.set_lenet_net_mode(2)
        assert np.array_equal(ctx.score(img), want_chain)
        # ... equals before the install; an install does not reset the mode, nor does set_lenet_weights
        ctx.set_lenet_net_mode(SPLIT)
        ctx.set_lenet_net(R.state(name))
        assert ctx.score(img).tobytes() == split.tobytes()
        ctx.set_lenet_torch(ltr.state(C))
        stock = ctx.score(img)
        out = np.zeros(2, np.float32)
        assert api.lib().gpd_hip_lenet_net_debug(ctx._h, 4, 1, out.ctypes.data) == -1  # the stock route ran
        ctx.set_lenet_net(R.state(name))
        assert ctx.score(img).tobytes() == split.tobytes()
    finally:
        ctx.close()
    fresh = _ctx(C)
    try:
        fresh.set_lenet_net_mode(SPLIT)  # before any network
        fresh.set_lenet_torch(ltr.state(C))
        assert np.array_equal(fresh.score(img), stock)
        fresh.set_lenet_net(R.state(name))
        assert fresh.score(img).tobytes() == split.tobytes()
    finally:
        fresh.close()


def test_reserve_then_batch_allocates_nothing_in_split_mode():
    """install, set the mode, THEN reserve: a batch within the reserved sizes books no growth of a scoring buffer on either lane —
    nothing beyond what the same clouds cause on the stock route"""
    name = "A"
    C = R.SHAPES[name][0]
    clouds = [synth.make_cloud(900 + cid, 2000 + 500 * cid) for cid in range(3)]
    samples = [synth.sample_indices(cl, 30 + 5 * cid) for cid, cl in enumerate(clouds)]
    sizes = dict(max_points=max(len(cl["xyz"]) for cl in clouds), max_cams=1, max_samples=max(len(s) for s in samples))
    net, stock = _ctx(C), _ctx(C)
    try:
        net.set_lenet_net(R.state(name))
        net.set_lenet_net_mode(SPLIT)
        stock.set_lenet_torch(ltr.state(C))
        allocs = {}
        for label, c in (("split", net), ("stock", stock)):
            c.reserve(**sizes)
            got = c.detect_batch(clouds, samples, 0)
            allocs[label] = [a for _, a in c.last_batch_timeline]
            c.detect_batch(clouds, samples, 0)
            allocs[label + ", second batch"] = [a for _, a in c.last_batch_timeline]
            assert all(nc >= 20 for _, _, nc, _ in got)
        print("allocs per cloud %s" % allocs)
        assert allocs["split"] == allocs["stock"], allocs
        assert allocs["split, second batch"] == [0, 0, 0] and allocs["stock, second batch"] == [0, 0, 0], allocs
        # a mode change voids the reservation of the scoring buffers, as an install does: they grow (booked) in the first pass
        net.set_lenet_net_mode(CHAIN)
        net.detect_batch(clouds, samples, 0)
        assert sum(a for _, a in net.last_batch_timeline) > 0
    finally:
        net.close()
        stock.close()


def test_every_entry_scores_in_split_mode():
    name = "A"
    cloud = synth.make_cloud(5, 2000)
    si = synth.sample_indices(cloud, 30)
    ctx = _split_ctx(name)
    try:
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
        # replay: the captured search -> images -> scores pass of the last detect
        ctx.detect(si)
        ctx.replay(2)
        _, lenet_ms, launches, sc = ctx.replay_times(n_scores=n_cand)
        assert launches == 1 and lenet_ms > 0 and np.array_equal(sc, want)
        ms = ctx.replay_kernel_ms()
        assert len(ms) == 4 and all(x > 0 for x in ms[:3]), ms
        # detect_sis: one round; its hands, handed to score_given, get the scores it reported
        lo, hi = cloud["xyz"].min(axis=0) - 0.5, cloud["xyz"].max(axis=0) + 0.5
        got = ctx.detect_sis(si, 1, 10, min_score=-3.0e38, workspace=(lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]), seed=3)
        hands = got["hands"]
        sets, slots = hands["set_index"], hands["slot"]
        given = np.zeros((got["num_sets"], ctx.n_slots), api.HAND_DTYPE)
        given[sets, slots] = hands
        first = np.unique(sets, return_index=True)[1]
        given["sample"][sets[first], 0] = hands["sample"][first]
        assert int(given["valid"].astype(bool).sum()) == len(hands) >= len(want)
        sis_scored, sis_scores, _, _ = ctx.score_given(given)  # (score_given equals score on the same images: above)
        assert np.array_equal(sis_scored[sets, slots]["score"], hands["score"])
        assert np.array_equal(np.sort(sis_scores), np.sort(hands["score"]))
        # the chain's scores of the same images differ somewhere, and not by much
        ctx.set_lenet_net_mode(CHAIN)
        chain = ctx.score(img)
        assert (chain != want).any() and np.abs(chain - want).max() < 1e-4
    finally:
        ctx.close()


def test_trainer_install_takes_the_mode():
    shape = R.ALL_SHAPES["A"]
    C = shape[0]
    img = R.images("A", 35)
    lab = (np.arange(35) % 2).astype(np.uint8)
    ctx, other = _ctx(C), _ctx(C)
    try:
        t = api.Trainer(ctx, api.train_default_params(C, 16), shape=shape[1:])
        try:
            t.set_data(img, lab)
            t.set_state(api.init_state(C, 9, shape=shape[1:]))
            t.steps(np.arange(32, dtype=np.int32).reshape(2, 16))
            st = t.get_state()
            t.install(other, net_mode=SPLIT)
            split = other.score(img)
            assert other.lenet_net_info()["scratch_bytes_per_image"] != 4 * (6 * 784 + 16 * 144 + 120 + 84 + 2)
            t.install(other)  # None leaves the context's mode alone
            assert other.score(img).tobytes() == split.tobytes()
            t.install(other, net_mode=CHAIN)
            chain = other.score(img)
        finally:
            t.close()
        ref = _ctx(C)
        try:
            ref.set_lenet_net(st, float(t.params.input_scale), net_mode=SPLIT)
            assert ref.score(img).tobytes() == split.tobytes()
        finally:
            ref.close()
        assert (chain != split).any() and np.abs(chain - split).max() <= 1e-4 * max(1.0, float(np.abs(chain).max()))
    finally:
        ctx.close()
        other.close()


def test_detect_grasps_cli_scores_in_split_mode(tmp_path):
    import torch
    from gpd_amd import torch_export
    from test_host_cli import CLI, _subsample_indices, _write_case
    name = "A"
    C, S, K = R.SHAPES[name][0], 30, 10
    cl = synth.make_cloud(5, 2000)
    st = R.state(name)
    cfg, pcd = _write_case(tmp_path, cl, ltr.eigen_weights(C), S, K, channels=C, extra="hip_lenet_net_mode = 1\n")
    params = tmp_path / "params"
    for f in os.listdir(str(params)):  # the Eigen-layout files _write_case wrote: this directory is a torch one
        os.remove(str(params / f))
    model = tmp_path / "model.pwf"
    torch.save({k: torch.from_numpy(v.copy()) for k, v in st.items()}, str(model))
    assert torch_export.main([str(model), str(params)]) == 0
    out = subprocess.run([CLI, str(cfg), str(pcd)], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "hip_lenet_net_mode: 1" in out.stdout
    got = np.array([float(l.split()[1]) for l in out.stdout.splitlines() if l.startswith("GRASP ")], np.float32)
    ctx = _split_ctx(name)
    try:
        ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
        idx = _subsample_indices(len(cl["xyz"]), S)
        sel, _, n_cand = ctx.detect_select(idx, K)
        sel = sel.copy()
        assert len(sel) == K and n_cand > K
        assert np.array_equal(got, sel["score"])
        ctx.set_lenet_net_mode(CHAIN)
        chain_sel, _, _ = ctx.detect_select(idx, K)
        assert (chain_sel["score"] != sel["score"]).any()
    finally:
        ctx.close()
