"""gpd_hip_train_create_net where test_gpu_train_net.py does not reach: Caffe's SGD rule on other widths and on ten
tensors, with multipliers at non-stock offsets; the batch edges behind NetCCFFF's third dense layer; a short batch after a long
one in one trainer; which head kernel is instantiated and its branches on fc3; the shapes at which fc1's partials size the
partial buffer; dead and nearly dead dense layers; eval, install and step_timed of such trainers.

Truth: torch in float64 on the CPU (train_net_ref.py).  Yardstick: its two float32 runs, factor 4, with train_ref.check_gradients'
floors; for the head, test_gpu_train_edges' _head_ok.  Each test asserts its condition on the reference first (the same conditions
run without a device in test_train_net_host.py).  Measured figures: profiles/NOTES.md §L.
"""
import time

import numpy as np
import pytest

import train_net_ref as nr
import train_ref as tr
from test_gpu_train_edges import F32_MIN_NORMAL, HEAD_ABS, HEAD_REL, _head_ok

pytestmark = pytest.mark.gpu


class _Rig:
    """A context and a trainer on it, closed in order."""

    def __init__(self, C_, **kw):
        from gpd_amd import api
        self.ctx = api.Context(api.default_params(C_))
        try:
            self.trainer = api.Trainer(self.ctx, api.train_default_params(C_, kw.pop("max_batch", 64)), kw.pop("recipe", None), **kw)
        except Exception:
            self.ctx.close()
            raise

    def __enter__(self):
        return self.trainer

    def __exit__(self, *exc):
        self.trainer.close()
        self.ctx.close()


def _same(a, b):
    return set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)


def _zero_bytes(a):
    return a.tobytes() == bytes(a.nbytes)


def _gradient_check(what, dims, st, img, lab, idx, max_batch, caffe=False):
    """train_net_ref.check_gradients of set (img, lab) gathered by idx under state st, every tensor's float64 gradient non-zero
    -> (gradients, loss, g64)"""
    from gpd_amd import api
    g64, l64, e32, el32 = nr.yardstick(st, img[idx], lab[idx], conv_relu=not caffe)
    assert all(np.abs(g).max() > 0 for g in g64.values()), {k: float(np.abs(g).max()) for k, g in g64.items()}
    recipe = api.train_default_recipe(0, network=api.NET_CAFFE) if caffe else None
    t0 = time.time()
    with _Rig(dims[0], max_batch=max_batch, recipe=recipe, shape=dims[1:]) as t:
        assert t.shape.as_tuple() == dims
        t.set_state(st)
        t.set_data(img, lab)
        got, loss = t.gradients(idx)
        again, loss2 = t.gradients(idx)
    worst = nr.check_gradients(what, got, loss, g64, l64, e32, el32)
    print("%s largest ratio %.2f, %.2f s on the device" % (what, worst, time.time() - t0))
    assert loss == loss2 and _same(got, again)
    return got, loss, g64


# ---- A. Caffe's SGD rule at other widths and on ten tensors -----------------------------------------------------------------------

@pytest.mark.parametrize("case", list(nr.SGD_CASES))
def test_sgd_trajectory_against_the_caffe_rule(case):
    """sgd_kernel counts eight slots: on ten tensors fc3.* take the rate and decay of fc2.bias's slot (every multiplier is 1
    there), on eight the ends of the slots are this shape's offsets: a frozen tensor comes back as the same bytes and both its
    neighbours in the buffer move, within allowance."""
    import train_caffe_ref as cr
    widths, st0, img, lab, rows, hyper, lr_mult, decay_mult = nr.sgd_case(case)
    l64, s64, el32, e32 = nr.sgd_trajectory_yardstick(st0, img, lab, rows, hyper, lr_mult, decay_mult)
    moved = nr.check_sgd_moves(case, st0, s64, lr_mult)
    recipe, kw = cr.recipe(hyper, lr_mult, decay_mult)
    t0 = time.time()
    with _Rig(3, max_batch=rows.shape[1], recipe=recipe, shape=widths, **kw) as t:
        t.set_state(st0)
        t.set_data(img, lab)
        losses = t.steps(rows)
        state = t.get_state()
    dt = time.time() - t0
    assert losses.shape == (len(rows),) and losses.dtype == np.float32 and tuple(state) == tuple(s64)
    bad, worst = [], 0.0
    for s in range(len(rows)):
        err, allow = abs(float(losses[s]) - l64[s]), max(nr.FACTOR * el32[s], 2.0 ** -21)
        print("%s step %d: loss f64 %.9g  device %.9g  e32 = %.3g  error = %.3g  allowance = %.3g" % (case, s, l64[s], losses[s], el32[s], err, allow))
        if err > allow:
            bad.append((s, err, allow))
    for k in s64:
        err = float(np.abs(state[k].astype(np.float64) - s64[k]).max())
        allow = max(nr.FACTOR * e32[k], float(np.spacing(np.float32(np.abs(s64[k]).max()))))
        ratio = err / e32[k] if e32[k] else 0.0
        worst = max(worst, ratio)
        print("%s %-12s e32 = %.3g  device error = %.3g  ratio = %.2f  allowance = %.3g  moved by %.3g" % (case, k, e32[k], err, ratio, allow, moved[k]))
        if err > allow:
            bad.append((k, err, allow))
        if lr_mult and k in lr_mult:
            assert state[k].tobytes() == st0[k].tobytes(), k  # frozen: the same bytes
        else:
            assert float(np.abs(state[k] - st0[k]).max()) > 1e-5, k
    print("%s: largest ratio %.2f, %.2f s on the device" % (case, worst, dt))
    assert not bad, bad


# ---- B. batch edges behind the third layer ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,caffe", [(B, False) for B in nr.BATCH_EDGES] + [(33, True)])
def test_batch_edges(B, caffe):
    """K = B in pairs (an odd B pads one), M = B in 32-row tiles, the chains b mod 8 at W = H2, head_kernel's blocks of 64 and
    block_sum's loop at 257: max_batch = B at widths that are no multiple of 2, 8 or 32."""
    from gpd_amd import api
    dims = nr.BATCH_DIMS
    st = api.init_state(dims[0], nr.BATCH_SEED, shape=dims[1:])
    what = "%s%s, B = %d:" % (dims, " (no conv ReLU)" if caffe else "", B)
    _gradient_check(what, dims, st, tr.images(1, n=257), tr.labels(257), nr.batch_indices(B, 257), B, caffe)


# ---- C. a short batch after a long one ----------------------------------------------------------------------------------------------

def test_short_batch_after_long():
    """d_a2, d_dz2, d_dz1 and the partials are sized by max_batch and keep a longer batch's rows: only the guards of the K = B
    sums and of the tile rows keep them out.  The same bytes as trainers that never saw a longer batch."""
    from gpd_amd import api
    dims = nr.BATCH_DIMS
    img, lab = tr.images(1, n=257), tr.labels(257)
    st = api.init_state(dims[0], nr.BATCH_SEED, shape=dims[1:])
    rows = np.stack([nr.batch_indices(9, 257), nr.batch_indices(9, 200)])
    fresh = {}
    for B in (9, 33):
        with _Rig(1, max_batch=B, shape=dims[1:]) as t:
            t.set_state(st)
            t.set_data(img, lab)
            fresh[B] = t.gradients(nr.batch_indices(B, 257))
            if B == 9:
                fresh["steps"] = (t.steps(rows), t.get_state())
    assert all(np.abs(g).max() > 0 for g in fresh[9][0].values()) and not _same(fresh[9][0], fresh[33][0])
    with _Rig(1, max_batch=257, shape=dims[1:]) as t:
        t.set_state(st)
        t.set_data(img, lab)
        long, long_loss = t.gradients(nr.batch_indices(257, 257))
        assert np.isfinite(long_loss) and all(np.abs(g).max() > 0 for g in long.values())
        for B in (9, 33):
            got, loss = t.gradients(nr.batch_indices(B, 257))
            assert loss == fresh[B][1] and _same(got, fresh[B][0]), B
        t.gradients(nr.batch_indices(257, 257))
        losses = t.steps(rows)
        assert losses.tobytes() == fresh["steps"][0].tobytes() and _same(t.get_state(), fresh["steps"][1])
    assert not _same(fresh["steps"][1], st)


# ---- D. which head kernel, and its branches on fc3 ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(3, 6, 16, 120, 500), (3, 6, 16, 500, 0), (3, 6, 16, 500, 84)])
def test_head_kernel_choice(dims):
    """The head of constant width 500 reading fc2's activations, the same at non-stock conv widths, and H1 = 500 in front of a
    third layer, where the head's width is 84."""
    from gpd_amd import api
    st = api.init_state(dims[0], 2, shape=dims[1:])
    _gradient_check("%s, B = 5:" % (dims,), dims, st, tr.images(dims[0]), tr.labels(), nr.batch_indices(5, 70), 5)


_ONE = np.float32(1.0)
HEAD_TARGETS = (1e-4, float(np.nextafter(_ONE, np.float32(0))), 1.0, float(np.nextafter(_ONE, np.float32(2))), 2.0, 17.4, 87.5, 103.5, 110.0)


@pytest.mark.parametrize("H2", [84, 500])
def test_head_probes_on_fc3(H2):
    """test_gpu_train_edges.test_head_probes at offset 0 on NetCCFFF (1; 3, 5, 33, H2): B = 1, one image resident under both
    labels, fc3.bias = (0, target - d0) puts the device's d = z1 - z0 on the target; the gradient read is fc3.bias's, which IS
    dlogits.  H2 = 84: head_kernel<0>, H2 = 500: head_kernel<500> on fc2's activations."""
    import torch
    from gpd_amd import api
    dims = (1, 3, 5, 33, H2)
    img = np.repeat(tr.images(1)[:1], 2, axis=0)
    lab = np.array([0, 1], np.uint8)
    st = api.init_state(1, 2, shape=dims[1:])
    z64 = nr.logits(dict(st, **{"fc3.bias": np.zeros(2, np.float32)}), img[:1], torch.float64)[0]
    assert abs(z64[1] - z64[0]) > 0  # fc2's activations reach the logits: the head's sums are not empty
    t0 = time.time()
    worst, bad, band, near_one = {"loss": 0.0, "grad": 0.0}, [], [], []
    with _Rig(1, max_batch=4, shape=dims[1:]) as t:
        t.set_data(img, lab)
        st["fc3.bias"] = np.zeros(2, np.float32)
        t.set_state(st)
        z = t.eval(np.array([0], np.int32))[0][0]
        d0 = float(z[1]) - float(z[0])
        assert abs(d0 - (z64[1] - z64[0])) <= 1e-4
        for target in HEAD_TARGETS:
            for sign in (1.0, -1.0):
                T = sign * target
                b1 = T - d0
                # around the cut the last bit of the logits decides the branch: step fc3.bias[1] by what is missing (twice at most)
                for attempt in range(3 if abs(target - 1) < 1e-6 else 1):
                    st["fc3.bias"] = np.array([0.0, b1], np.float32)
                    t.set_state(st)
                    z = t.eval(np.array([0], np.int32))[0][0]
                    d32 = np.float32(z[1]) - np.float32(z[0])  # the kernel's d: one float32 subtraction
                    if float(d32) == float(np.float32(T)):
                        break
                    b1 += T - float(d32)
                ulp = float(np.spacing(np.float32(max(abs(float(z[0])), abs(float(z[1])), abs(T)))))
                assert abs(float(d32) - T) <= 64 * ulp, (T, z)
                if abs(target - 1) < 1e-6:
                    near_one.append(abs(float(d32)))
                d64, loss64, p64 = tr.head64(np.stack([z, z]), lab)
                for i in (0, 1):
                    g, loss = t.gradients(np.array([i], np.int32))
                    gb = g["fc3.bias"]
                    ok_l, f_l = _head_ok(loss, float(loss64[i]), d32)
                    ok_g, f_g = _head_ok(abs(float(gb[1])), float(p64[i]), d32)
                    # antisymmetric by construction, the true class pulled up
                    ok_s = gb[0] == -gb[1] and abs(float(gb[0])) == abs(float(gb[1])) and (gb[1] <= 0 if lab[i] else gb[1] >= 0)
                    if not (ok_l and ok_g and ok_s):
                        bad.append((T, int(lab[i]), float(d32), loss, float(loss64[i]), gb.tolist(), float(p64[i])))
                    worst["loss"], worst["grad"] = max(worst["loss"], f_l), max(worst["grad"], f_g)
                    if 0 < min(loss64[i], p64[i]) < F32_MIN_NORMAL:
                        band.append((T, int(lab[i]), loss, float(loss64[i]), abs(float(gb[1])), float(p64[i])))
                    # the same image four times: / 4 and the four adds give p_false back exactly while p_false / 4 is a normal float32
                    if min(p64[i], loss64[i]) >= 2.0 ** -120:
                        g4, loss4 = t.gradients(np.array([i] * 4, np.int32))
                        if g4["fc3.bias"].tobytes() != gb.tobytes() or loss4 != loss:
                            bad.append(("four times", T, int(lab[i]), g4["fc3.bias"].tolist(), gb.tolist(), loss4, loss))
    for row in band:
        print("H2 = %d underflow band: d = %g, label %d: loss %.9g (f64 %.9g), |grad| %.9g (f64 %.9g)" % ((H2,) + row))
    print("H2 = %d: %d probes, largest fraction of the bound: loss %.3f, gradient %.3f; %.1f s"
          % (H2, 4 * len(HEAD_TARGETS), worst["loss"], worst["grad"], time.time() - t0))
    assert not bad, bad
    # both sides of the cut were visited, each within 2^-20 of it
    assert min(near_one) < 1 <= max(near_one) and max(abs(v - 1) for v in near_one) <= 2.0 ** -20, near_one


def test_both_head_branches_in_one_batch():
    st, d = nr.both_branches_state()
    B = nr.HEAD_B
    print("margins:", np.array2string(np.sort(d), precision=3), "labels", tr.labels()[:B].tolist())
    _gradient_check("%s, B = 16, both branches:" % (nr.HEAD_DIMS,), nr.HEAD_DIMS, st, tr.images(3)[:B], tr.labels()[:B], np.arange(B, dtype=np.int32), B)


def test_saturated_batch():
    st, d = nr.saturated_state()
    B = nr.HEAD_B
    print("margins:", np.array2string(np.sort(d), precision=1), "labels", tr.labels()[:B].tolist())
    _gradient_check("%s, B = 16, every |d| > 50:" % (nr.HEAD_DIMS,), nr.HEAD_DIMS, st, tr.images(3)[:B], tr.labels()[:B], np.arange(B, dtype=np.int32), B)


# ---- E. the third term of the partial buffer ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", list(nr.PART_DIMS))
def test_fc1_partials_size_the_partial_buffer(dims):
    """max_batch * 16 H1 floats of fc1's forward partials are the largest use of the partial buffer here, 80 times the next
    (test_train_net_host.test_which_term_sizes_the_partial_buffer).  A test cannot prove a buffer's size: what this checks is that
    all 16 ranges of every image arrive in fc1's sum, which a buffer sized by the convolutions' terms alone could not hold."""
    from gpd_amd import api
    a, b, c = nr.part_terms(dims)
    assert c > a and c > b
    st = api.init_state(dims[0], 2, shape=dims[1:])
    _gradient_check("%s, B = 5:" % (dims,), dims, st, tr.images(dims[0]), tr.labels(), nr.batch_indices(5, 70), 5)


# ---- F. dead and nearly dead dense layers -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layer", ["fc2", "fc1"])
def test_dead_layer(layer):
    """Every unit of the layer clamped on every image: ActMaskStore, fc2_back_kernel and the K = B sums get nothing but zeros, and
    every gradient that hangs on the layer's output is zero in all its bytes.  fc2 dead: the logits ARE fc3.bias, so the loss and
    fc3.bias's gradient are the head's own arithmetic, held to the head's allowance (_head_ok's terms; in a sum of B terms each
    term keeps its relative bound, so the sum keeps it of the sum of the magnitudes)."""
    Cn = nr.DEAD_DIMS[0]
    img, lab, idx = tr.images(Cn), tr.labels(), nr.DEAD_IDX
    st = nr.dead_state(layer)
    g64, l64, e32, el32 = nr.yardstick(st, img[idx], lab[idx])
    nr.check_dead_reference(layer, None, g64)
    with _Rig(Cn, max_batch=len(idx), shape=nr.DEAD_DIMS[1:]) as t:
        t.set_state(st)
        t.set_data(img, lab)
        got, loss = t.gradients(idx)
        logits, _ = t.eval(idx)
    for k in got:
        if k not in nr.DEAD_NONZERO[layer]:
            assert _zero_bytes(got[k]), (k, float(np.abs(got[k]).max()))
    if layer == "fc1":  # fc2's units see their biases alone: what is left goes through the yardstick
        nr.check_gradients("fc1 dead:", got, loss, g64, l64, e32, el32)
        return
    assert all(z.tobytes() == st["fc3.bias"].tobytes() for z in logits)
    d32 = np.float32(st["fc3.bias"][1]) - np.float32(st["fc3.bias"][0])
    assert abs(float(d32)) > 1e-3
    _, loss64, p64 = tr.head64(logits, lab[idx])
    rel = float(np.spacing(np.float32(abs(d32)))) / 2 + HEAD_REL
    sign = np.where(lab[idx] == 1, -1.0, 1.0)  # the sign of dlogits[1]: the true class is pulled up
    want = float((sign * p64).sum()) / len(idx)
    for what, dev, ref, mag in (("loss", loss, float(loss64.mean()), float(loss64.mean())),
                                ("fc3.bias[1]", float(got["fc3.bias"][1]), want, float(p64.sum()) / len(idx)),
                                ("fc3.bias[0]", float(got["fc3.bias"][0]), -want, float(p64.sum()) / len(idx))):
        err, allow = abs(dev - ref), mag * rel + HEAD_ABS
        print("fc2 dead %s: f64 %.9g  device %.9g  error = %.3g  allowance = %.3g (%.3f of it); torch's own float32 error %.3g"
              % (what, ref, dev, err, allow, err / allow, el32 if what == "loss" else e32["fc3.bias"]))
        assert err <= allow, (what, dev, ref, allow)
    assert abs(want - float(g64["fc3.bias"][1])) <= 1e-6 * abs(want) + 1e-12 and abs(float(loss64.mean()) - l64) <= 1e-6 * l64


@pytest.mark.parametrize("layer,live", [("fc2", 37), ("fc1", 53)])
def test_one_live_unit(layer, live):
    Cn = nr.DEAD_DIMS[0]
    img, lab, idx = tr.images(Cn), tr.labels(), nr.DEAD_IDX
    st = nr.dead_state(layer, live)
    g64, l64, e32, el32 = nr.yardstick(st, img[idx], lab[idx])
    nr.check_dead_reference(layer, live, g64)
    with _Rig(Cn, max_batch=len(idx), shape=nr.DEAD_DIMS[1:]) as t:
        t.set_state(st)
        t.set_data(img, lab)
        got, loss = t.gradients(idx)
    worst = nr.check_gradients("%s, unit %d alone live:" % (layer, live), got, loss, g64, l64, e32, el32)
    print("%s, unit %d alone live: largest ratio %.2f" % (layer, live, worst))
    w = got[layer + ".weight"]
    assert np.flatnonzero(np.abs(w).max(axis=1) > 0).tolist() == [live]
    assert _zero_bytes(np.delete(w, live, axis=0)) and _zero_bytes(np.delete(got[layer + ".bias"], live))
    assert got[layer + ".bias"][live] != 0


# ---- G. eval ----------------------------------------------------------------------------------------------------------------------------

def test_eval_chunks_sets_and_ties():
    """test_gpu_train_edges.test_eval_chunks_sets_and_ties through fc2's forward GEMM: 70 images at max_batch 64."""
    dims, n = (3, 6, 16, 120, 84), 70
    img, lab = tr.images(3), tr.labels()
    st, truth, e32 = nr.eval_state()
    assert nr.HEAD_DIMS == dims
    rev = np.arange(n)[::-1]
    perm = np.random.RandomState(21).randint(0, n, n).astype(np.int32)  # with repeats
    perm[[0, 63, 64, 69]] = [69, 5, 5, 0]  # image 5 on both sides of the chunk boundary
    assert len(set(perm.tolist())) < n
    with _Rig(3, max_batch=64, shape=dims[1:]) as t:
        t.set_state(st)
        t.set_data(img, lab)
        t.set_data(img[::-1], lab[::-1], which=1)
        first = {w: t.eval(n=n, which=w) for w in (0, 1)}          # chunks of 64 + 6
        listed = {w: t.eval(perm, which=w) for w in (0, 1)}
        alone = [t.eval(np.array([i], np.int32))[0][0] for i in (0, 5, 63, 64, 69)]
        tie = {k: np.array(v) for k, v in st.items()}
        tie["fc3.weight"][:] = 0
        tie["fc3.bias"][:] = 0.25
        t.set_state(tie)
        tied = {w: t.eval(n=n, which=w) for w in (0, 1)}
    for w, order in ((0, np.arange(n)), (1, rev)):
        for what, (logits, correct), ids in (("first 70", first[w], order), ("listed", listed[w], order[perm])):
            assert logits.shape == (n, 2) and logits.dtype == np.float32
            err = float(np.abs(logits - truth[ids]).max())
            print("eval set %d %s: |logits - f64| = %.3g, float32 forward error %.3g, ratio %.2f, %d correct" % (w, what, err, e32, err / e32, correct))
            assert err <= 4 * e32
            assert correct == int(((logits[:, 1] > logits[:, 0]) == (lab[ids] == 1)).sum())
            assert correct == int(((truth[ids, 1] > truth[ids, 0]) == (lab[ids] == 1)).sum())
            # an image's logits are the same bytes wherever it stands
            assert logits.tobytes() == first[0][0][ids].tobytes(), (w, what)
        logits, correct = tied[w]
        assert (logits == 0.25).all() and correct == int((lab == 0).sum())  # a tie predicts class 0, as torch.max
    for i, z in zip((0, 5, 63, 64, 69), alone):
        assert z.tobytes() == first[0][0][i].tobytes(), i
    assert 0 < int((lab == 0).sum()) < n


# ---- H. install -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims,caffe,scale", [((3, 7, 9, 33, 0), True, 1.0 / 256), ((3, 6, 16, 120, 84), False, 1.0 / 255)])
def test_install_closes_the_loop(dims, caffe, scale):
    """A few steps, then Trainer.install onto the context's general route: its score and eval's logit1 - logit0 are two float32
    summation orders of one network, 4 e32 apart at the most, and eval is as close to float64."""
    from gpd_amd import api
    img, lab = tr.images(3), tr.labels()
    rows = (np.arange(15, dtype=np.int32).reshape(3, 5) * 3) % len(lab)
    recipe, lr = (api.train_default_recipe(1), api.CAFFE_BASE_LR) if caffe else (None, 1e-3)
    st0 = nr.xavier_state(3, dims[1:]) if caffe else api.init_state(3, 2, shape=dims[1:])
    with _Rig(3, max_batch=64, recipe=recipe, shape=dims[1:], lr=lr, input_scale=scale) as t:
        t.set_state(st0)
        t.set_data(img, lab)
        losses = t.steps(rows)
        state = t.get_state()
        logits, _ = t.eval(n=len(img))
        ctx = t._ctx
        t.install()
        info = ctx.lenet_net_info()
        score = ctx.score(img)
    assert np.isfinite(losses).all() and any(not np.array_equal(state[k], st0[k]) for k in state)
    assert info["chunk_images"] > 0 and info["macs_per_image"] > 0
    truth, _, e32 = nr.logits_e32(state, img, scale, conv_relu=not caffe)
    t64 = truth[:, 1] - truth[:, 0]
    assert np.abs(t64).max() > 1e-3
    dev = logits[:, 1].astype(np.float64) - logits[:, 0]
    err, err64 = float(np.abs(score.astype(np.float64) - dev).max()), float(np.abs(dev - t64).max())
    print("%s%s at 1/%g: |score - (logit1 - logit0)| = %.3g, |eval - f64| = %.3g, e32 = %.3g, ratios %.2f and %.2f"
          % (dims, " (no conv ReLU)" if caffe else "", 1 / scale, err, err64, e32, err / e32, err64 / e32))
    assert err <= 4 * e32 and err64 <= 4 * e32


# ---- I. step_timed with a third layer -----------------------------------------------------------------------------------------------------

THIRD_NAMES = ["conv1_forward", "conv2_forward", "fc1_forward", "fc1_sum_relu", "fc2_forward", "head", "loss", "fc3_backward", "head_grads",
               "fc2_dw", "fc2_dx", "fc1_db", "fc1_dw", "fc1_dx", "conv2_db", "conv2_dw", "conv2_dw_sum", "conv2_dx", "conv1_db", "conv1_dw",
               "conv1_dw_sum"]


@pytest.mark.parametrize("solver", ["adam", "sgd"])
def test_step_timed_with_a_third_layer(solver):
    from gpd_amd import api
    dims, B = (3, 6, 16, 120, 84), 5
    img, lab = tr.images(3), tr.labels()
    rows = (np.arange(3 * B, dtype=np.int32).reshape(3, B) * 3) % len(lab)
    recipe, lr = (None, 1e-3) if solver == "adam" else (api.train_default_recipe(1), api.CAFFE_BASE_LR)
    st = api.init_state(3, 2, shape=dims[1:])
    want = THIRD_NAMES + [solver]
    assert len(want) == 22 and len(set(want)) == 22 and all(want)
    with _Rig(3, max_batch=B, recipe=recipe, shape=dims[1:], lr=lr) as t:
        t.set_data(img, lab)
        t.set_state(st)
        t.steps(rows)
        stepped, stepped_solver = t.get_state(), t.get_solver_state()
        t.set_state(st)
        for row in rows:
            times = t.step_timed(row)
            assert [n for n, _ in times] == want
            assert all(np.isfinite(ms) and ms >= 0 for _, ms in times), times
        timed, timed_solver = t.get_state(), t.get_solver_state()
    assert _same(stepped, timed) and not _same(stepped, st)
    assert stepped_solver["count"] == timed_solver["count"] == 3 and _same(stepped_solver["m"], timed_solver["m"])
