"""LeNet and the fused path where the other GPU tests do not reach: past one pass of lenet_forward, past candidate 79 537
(where a 32-bit byte offset into the 15-channel images wraps a second time), and at hostile weights in the split mode.

A. gpd_hip_score past one pass (gpd_amd/csrc/lenet.hip: passes of 65536 images that share scratch sized for one pass, the
second pass reading its images and writing its scores at an offset, the two image counters re-zeroed).  Every image of a large batch must get, bit for bit, the score it gets in a batch of 64 on the same context — the project's
claim that a score does not depend on the batch — and the small-batch scores are what the other GPU tests tie to numpy and
to the oracle.  The batch is pool[idx] for a random idx, so neighbours differ across the pass boundary and a score written
to, or an image read from, the wrong place shows.  In f32-chain mode three positions of the second pass (first, middle,
last) are also compared with the oracle's score of that image alone.

B. gpd_hip_detect / replay / detect_select / detect_sharded on more than 80 000 candidates of the 300k-point clutter cloud.

C. Weight sets made to stress the split path's operand splits (per-filter fixed-point position, digit-plane extremes, bf16
pieces of wide dynamic range, the conv2 route of filters 48 and 49, a cancelling ip1 unit), stage by stage on the device's
own previous stage, each output held against float64 RELATIVE TO ITS OWN sum of magnitudes."""
import os
import time

import numpy as np
import pytest

import lenet_ref
from gpd_amd import api, synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
PASS = 65536  # lenet_forward's kChunk


def _weights(C):
    g = os.path.join(GOLD, "lenet%d_params.npz" % C)
    return synth.lenet_weights(C, real=dict(np.load(g)) if os.path.exists(g) else None, trained_magnitude=True)


def _pool(rng, C, n=512):
    """512 distinct images of mixed sparsity, some with empty channels, an all-zero and an all-255 image among them
    (test_gpu_lenet_stress.py's pool, the two extremes made certain)."""
    base = np.zeros((n, 60, 60, C), np.uint8)
    for i in range(n):
        dens = rng.choice([0.0, 0.01, 0.05, 0.3, 1.0])
        base[i] = rng.randint(0, 256, (60, 60, C)) * (rng.rand(60, 60, C) < dens)
        if rng.rand() < 0.3:
            base[i, :, :, rng.randint(C):] = 0
        if rng.rand() < 0.05:
            base[i] = 255
    base[0] = 0
    base[1] = 255
    return base


def _small_batch_scores(ctx, base):
    ref = np.concatenate([ctx.score(base[i:i + 64]) for i in range(0, len(base), 64)])
    assert np.isfinite(ref).all() and len(np.unique(ref)) > len(base) // 3  # distinct enough that a misplaced score shows
    return ref


def _check_large(ctx, oracle_mod, w, base, ref, batch, n, rng, chain):
    idx = rng.randint(0, len(base), n)
    np.take(base, idx, axis=0, out=batch[:n])
    got = ctx.score(batch[:n])
    bad = np.flatnonzero(got != ref[idx])
    assert len(bad) == 0, (n, len(bad), bad[:8].tolist())
    if chain and n > PASS:
        for pos in sorted({PASS, PASS + (n - PASS) // 2, n - 1}):
            assert np.array_equal(got[pos:pos + 1], oracle_mod.lenet(batch[pos:pos + 1], w)), (n, pos)


def _check_small_after(ctx, base, ref, rng):
    # the scratch is at its largest now and still holds the rows of the large batch
    for n in (1, 17, 255):
        idx = rng.randint(0, len(base), n)
        assert np.array_equal(ctx.score(base[idx]), ref[idx]), n


@pytest.mark.parametrize("mode", [api.LENET_SPLIT, api.LENET_F32_CHAIN], ids=["split", "chain"])
@pytest.mark.parametrize("C", [1, 3])
def test_score_across_pass_boundaries(oracle_mod, C, mode):
    rng = np.random.RandomState(500 + C)
    w = _weights(C)
    base = _pool(rng, C)
    sizes = (PASS - 1, PASS, PASS + 1, PASS + 37, 2 * PASS + 1)
    batch = np.empty((max(sizes), 60, 60, C), np.uint8)  # 1.4 GB at three channels
    ctx = api.Context(api.default_params(C))
    try:
        ctx.set_lenet_weights(w)
        ctx.set_lenet_mode(mode)
        ref = _small_batch_scores(ctx, base)
        for n in sizes:
            _check_large(ctx, oracle_mod, w, base, ref, batch, n, rng, mode == api.LENET_F32_CHAIN)
        _check_small_after(ctx, base, ref, rng)
    finally:
        ctx.close()


def test_score_across_a_pass_boundary_15_channels(oracle_mod):
    """The shipped geometry: 65536 + 17 images of 54000 bytes (3.5 GB on the host, twice that on the device, built once),
    the default split mode and then the f32-chain mode on the same batch."""
    C, n = 15, PASS + 17
    rng = np.random.RandomState(515)
    w = _weights(C)
    base = _pool(rng, C)
    batch = np.empty((n, 60, 60, C), np.uint8)
    ctx = api.Context(api.default_params(C))
    try:
        ctx.set_lenet_weights(w)
        for mode in (api.LENET_SPLIT, api.LENET_F32_CHAIN):
            ctx.set_lenet_mode(mode)
            ref = _small_batch_scores(ctx, base)
            _check_large(ctx, oracle_mod, w, base, ref, batch, n, rng, mode == api.LENET_F32_CHAIN)
            _check_small_after(ctx, base, ref, rng)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# B. the fused path past 65536 and past 79 537 candidates
# ---------------------------------------------------------------------------------------------------------------------
N_SAMPLES = 25500  # the oracle's search + filter_workspace on this cloud: 62 577 candidates from 19 000 samples, 84 253 from 25 500
RECORD_F64 = ("frame", "position", "top", "bottom", "center", "grasp_width", "sample")
RECORD_INT = ("finger_placement_index", "half_antipodal", "full_antipodal")


def _same_as_oracle(got, want):
    """_full_compare's rule (test_gpu_configs.py) with the scores bit-identical: the f32-chain mode is the checker mode"""
    assert np.array_equal(got["valid"], want["valid"])
    v = want["valid"].astype(bool)
    for f in RECORD_INT + RECORD_F64 + ("score",):
        assert np.array_equal(got[f][v], want[f][v]), f
    return int(v.sum())


def test_fused_path_beyond_80000_candidates(oracle_mod):
    """synth.make_cloud(1234, 300000, clutter=True), 15 channels, 25 500 samples (about 84 000 candidates; 180 000 object points
    to draw from).  The 54 000-byte images of candidates 39 768 and 79 537 start past 2^31 and 2^32 bytes; two LeNet passes.

    Oracle comparison: the FULL form, every one of the 84 253 candidates against oracle.detect of all the samples — 18 s of wall
    time on the 16 CPUs of the measured run (printed by the test; profiles/lenet_limits.txt)."""
    cl = synth.make_cloud(1234, 300000, clutter=True)
    si = synth.sample_indices(cl, N_SAMPLES)
    assert len(si) == N_SAMPLES
    w = _weights(15)
    p = oracle_mod.default_params(15)
    cloud = (cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])
    ctxs = [api.Context(api.default_params(15)) for _ in range(3)]
    ctx = ctxs[0]
    try:
        for c in ctxs:
            c.set_lenet_weights(w)
        ctx.set_lenet_mode(api.LENET_F32_CHAIN)
        ctx.upload_cloud(*cloud)
        hands, n_cand = ctx.detect(si)
        hands = hands.copy()
        passes = ctx.fallbacks()["lenet_passes"]
        print("fused path: n_cand = %d, lenet_passes = %d" % (n_cand, passes))
        assert n_cand >= 80000, n_cand
        assert passes >= 2
        chain_scores = hands["score"][hands["valid"].astype(bool)]
        assert len(chain_scores) == n_cand
        # 5. the replay the benchmark times
        ctx.replay(3)
        ctx.replay(3)
        _, _, launches, sc = ctx.replay_times(n_scores=n_cand)
        assert launches == 2 and np.array_equal(sc, chain_scores)
        # 1. against the oracle
        t0 = time.time()
        oh, on, _ = oracle_mod.detect(p, *cloud, si, w)
        assert on == n_cand and _same_as_oracle(hands, oh) == n_cand
        print("fused path: all %d candidates compared with oracle.detect in %.0f s" % (n_cand, time.time() - t0))
        # 3. the default mode on the same context
        ctx.set_lenet_mode(api.LENET_SPLIT)
        split, n2 = ctx.detect(si)
        split = split.copy()
        assert n2 == n_cand
        v = hands["valid"].astype(bool)
        assert np.abs(split["score"][v] - hands["score"][v]).max() <= 1e-4
        a, b = split.copy(), hands.copy()
        a["score"] = 0
        b["score"] = 0
        assert a.tobytes() == b.tobytes()
        # 4. three shards that never cross a pass or an offset boundary: an independent route to the same bytes
        allc, ns, nc = ctx.detect_select(si, 0)
        allc = allc.copy()
        assert nc == n_cand == len(allc) and np.array_equal(allc["score"], split["score"][v])
        got, info = ctx.detect_sharded(ctxs[1:], cl, si)
        print("fused path: shards of %s candidates" % [i[1] for i in info])
        assert all(0 < i[1] < 39768 for i in info) and sum(i[1] for i in info) == n_cand
        assert got.tobytes() == allc.tobytes()
        # 6. selectGrasps
        sel, _, _ = ctx.detect_select(si, 100)
        want = oracle_mod.select(allc["score"], 100)
        assert np.array_equal(want, np.argsort(-allc["score"], kind="stable")[:100])
        assert sel.tobytes() == allc[want].tobytes()
    finally:
        for c in ctxs:
            c.close()


# ---------------------------------------------------------------------------------------------------------------------
# C. hostile weights, split mode
# ---------------------------------------------------------------------------------------------------------------------
U_SMALL, U_BIG, U_ZERO, U_CANCEL = 7, 77, 177, 277  # ip1 units
K_IMG = 5                                            # the image the cancelling unit's signs are chosen on


def _hostile_images(rng, C, n):
    img = _pool(rng, C, n)
    img[2] = rng.randint(0, 256, (60, 60, C))
    img[3] = 255
    img[4] = 0
    img[K_IMG] = rng.randint(1, 256, (60, 60, C))
    return img


def _ref64(img, w, C):
    """float64 forward with the weights as given (no fixed point, no pieces): pool1 [n,20,28,28], flat [n,7200]"""
    c1 = w["c1w"].reshape(20, C, 5, 5).astype(np.float64)
    c2 = w["c2w"].reshape(50, 20, 5, 5).astype(np.float64)
    p1 = np.empty((len(img), 20, 28, 28))
    flat = np.empty((len(img), 7200))
    for i in range(len(img)):
        x = np.transpose(img[i], (2, 0, 1)).astype(np.float64)
        p1[i] = lenet_ref.pool(lenet_ref.conv_valid(x, c1)) + w["c1b"].astype(np.float64)[:, None, None]
        h = lenet_ref.pool(lenet_ref.conv_valid(p1[i], c2)) + w["c2b"].astype(np.float64)[:, None, None]
        flat[i] = np.transpose(h, (1, 2, 0)).reshape(-1)
    return p1, flat


def _hostile_weights(C, big, img):
    """(weights, float64 reference intermediates of img).  conv1: filter 3 spanning e^-12..1, filter 7 with a lone 1e4, filter 11
    zero, filters 0 / 1 all +0.25 / -0.25 (largest weight an exact power of two, the extreme digit-plane sums), filter 19 with its
    largest weight -(2 - 2^-23) (top of a binade, negative); conv2: filters 48, 49 times 2^-10 or 2^10, filter 16 spanning
    e^-12..1, filter 33 zero; ip1: unit 7 times 2^-12, unit 77 times 2^8, unit 177 zero, unit 277's signs arranged so that its
    sum on image K_IMG cancels."""
    rng = np.random.RandomState(900 + C)
    w = {k: v.copy() for k, v in synth.lenet_weights(C, seed=11, trained_magnitude=True).items()}
    K = C * 25
    c1 = w["c1w"].reshape(20, K)
    c1[3] *= np.exp(rng.uniform(-12, 0, K)).astype(np.float32)
    c1[7, 5] = 1e4
    c1[11] = 0
    c1[0] = 0.25
    c1[1] = -0.25
    c1[19, np.abs(c1[19]).argmax()] = np.float32(-(2.0 - 2.0 ** -23))
    assert np.abs(c1[19]).max() == np.float32(2.0 - 2.0 ** -23) and c1[19].min() == -np.abs(c1[19]).max()
    c2 = w["c2w"].reshape(50, 500)
    c2[48:50] *= np.float32(2.0 ** (10 if big else -10))
    c2[16] *= np.exp(rng.uniform(-12, 0, 500)).astype(np.float32)
    c2[33] = 0
    f1 = w["f1w"].reshape(7200, 500)
    f1[:, U_SMALL] *= np.float32(2.0 ** -12)
    f1[:, U_BIG] *= np.float32(2.0 ** 8)
    f1[:, U_ZERO] = 0
    p1, flat = _ref64(img, w, C)
    # the cancelling unit: largest terms first, every product given the sign that opposes the running sum
    x, a = flat[K_IMG], np.abs(f1[:, U_CANCEL]).astype(np.float64)
    t = np.abs(x) * a
    run = float(w["f1b"][U_CANCEL])
    sgn = np.ones(7200)
    for k in np.argsort(-t):
        s = -1.0 if run > 0 else 1.0
        run += s * t[k]
        sgn[k] = s if x[k] >= 0 else -s
    f1[:, U_CANCEL] = (sgn * a).astype(np.float32)
    assert abs(x @ f1[:, U_CANCEL].astype(np.float64) + w["f1b"][U_CANCEL]) <= 2.0 ** -10 * (t.sum() + abs(w["f1b"][U_CANCEL]))
    return w, p1, flat


def _stage_errors(got, ref, chain, S, N, what):
    """got / chain / ref / S componentwise.  1. the derived bound: f32 accumulation of N exact products in ANY order errs by at
    most about N 2^-24 S, the three dropped piece products (m l, l m, l l) by less than 3 2^-24 of a term, the bias add by
    2^-24 of the result.  2. E = max |err| / S for the device and for the k-ascending f32 fmaf chain on the same inputs."""
    assert (S > 0).all()
    err = np.abs(got - ref)
    worst = int(np.argmax(err / S))
    assert (err <= (N + 4) * 2.0 ** -24 * S).all(), (what, worst, float(err.flat[worst]), float(S.flat[worst]))
    return float((err / S).max()), float((np.abs(chain - ref) / S).max())


@pytest.mark.parametrize("n", [37, 80])
@pytest.mark.parametrize("big", [False, True], ids=["f48x2^-10", "f48x2^10"])
@pytest.mark.parametrize("C", [15, 12, 3, 1])
def test_hostile_weights_stage_by_stage(oracle_mod, C, big, n):
    rng = np.random.RandomState(700 + C)
    img = _hostile_images(rng, C, n)
    w, p1_64, flat_64 = _hostile_weights(C, big, img)
    c2w64 = w["c2w"].reshape(50, 20, 5, 5).astype(np.float64)
    f1w64 = w["f1w"].reshape(7200, 500).astype(np.float64)
    c2b64, f1b64 = w["c2b"].astype(np.float64), w["f1b"].astype(np.float64)
    # the inputs stay inside the kernels' exactness argument: finite everywhere, no subnormal bf16 piece
    ip1_64 = flat_64 @ f1w64 + f1b64
    for a in (p1_64, flat_64, ip1_64):
        assert np.isfinite(a.astype(np.float32)).all()
    for a in (w["c2w"], w["f1w"], p1_64.astype(np.float32), flat_64.astype(np.float32)):
        assert not lenet_ref.has_subnormal_piece(a)
    ctx = api.Context(api.default_params(C))
    try:
        ctx.set_lenet_weights(w)
        ctx.set_lenet_mode(api.LENET_SPLIT)
        sc = ctx.score(img)
        pool1 = ctx.lenet_debug(0, n).reshape(n, 28, 28, 20)
        xs = ctx.lenet_debug(1, n)
        fc1t = ctx.lenet_debug(2, n)
        assert np.isfinite(sc).all()
        # conv1 + pool1: exact, every image
        for i in range(n):
            assert np.array_equal(pool1[i], lenet_ref.pool1_exact(img[i], w, C)), i
        # the pieces are a split of an f32
        flat = lenet_ref.bf16_to_f64(xs[0]) + lenet_ref.bf16_to_f64(xs[1]) + lenet_ref.bf16_to_f64(xs[2])
        assert np.array_equal(flat.astype(np.float32).astype(np.float64), flat)
        assert not lenet_ref.has_subnormal_piece(pool1) and not lenet_ref.has_subnormal_piece(flat.astype(np.float32))
        # conv2 + pool2 on the device's own pool1; a pooled output errs by at most the largest error of its window
        ref2, S2, ch2 = np.empty((n, 7200)), np.empty((n, 7200)), np.empty((n, 7200))
        c2w4 = w["c2w"].reshape(50, 20, 5, 5)
        for i in range(n):
            x = np.ascontiguousarray(np.transpose(pool1[i], (2, 0, 1)))
            x64 = x.astype(np.float64)
            h = lenet_ref.pool(lenet_ref.conv_valid(x64, c2w64)) + c2b64[:, None, None]
            s = lenet_ref.pool(lenet_ref.conv_valid(np.abs(x64), np.abs(c2w64))) + np.abs(c2b64)[:, None, None]
            c = lenet_ref.pool(oracle_mod.conv_generic(x, c2w4, w["c2b"]).astype(np.float64))
            ref2[i], S2[i], ch2[i] = (np.transpose(a, (1, 2, 0)).reshape(-1) for a in (h, s, c))
        e2 = _stage_errors(flat, ref2, ch2, S2, 6 * 512, "conv2")
        # ip1 + ReLU on the device's own flat (ReLU does not increase an error)
        ref3 = np.maximum(flat @ f1w64 + f1b64, 0.0)
        S3 = np.abs(flat) @ np.abs(f1w64) + np.abs(f1b64)
        wt = np.ascontiguousarray(w["f1w"].reshape(7200, 500).T).reshape(500, 7200, 1, 1)
        flat32 = flat.astype(np.float32)
        ch3 = np.stack([np.maximum(oracle_mod.conv_generic(flat32[i].reshape(7200, 1, 1), wt, w["f1b"]).reshape(500), 0.0)
                        for i in range(n)]).astype(np.float64)
        e3 = _stage_errors(fc1t.T.astype(np.float64), ref3, ch3, S3, 6 * 7296, "ip1")
        print("lenet_limits C=%2d %-9s n=%2d  conv2: E_split %.3g  E_chain %.3g   ip1: E_split %.3g  E_chain %.3g"
              % (C, "f48x2^10" if big else "f48x2^-10", n, e2[0], e2[1], e3[0], e3[1]))
        assert e2[0] <= 2 * e2[1], ("conv2", e2)
        assert e3[0] <= 2 * e3[1], ("ip1", e3)
        # ip2 on the device's own ip1
        f2 = w["f2w"].astype(np.float64)
        y = fc1t.T.astype(np.float64)
        ref = (y @ f2[1::2] + w["f2b"][1]) - (y @ f2[0::2] + w["f2b"][0])
        assert np.abs(sc - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
        # the same weights through the f32 chain: the oracle, bit for bit
        ctx.set_lenet_mode(api.LENET_F32_CHAIN)
        assert np.array_equal(ctx.score(img), oracle_mod.lenet(img, w))
    finally:
        ctx.close()
