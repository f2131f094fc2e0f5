"""conv1's tile epilogue and conv2's piece split on the device (gpd_amd/csrc/lenet_fast.hip), bit for bit.

conv1 rounds the four exact sums of a pool window to f32 and THEN takes their maximum across a lane quad (two DPP-fused
v_max_f32), the x - 128 correction rides in the digit sums' start value, and the stores go through a scalar base.  pool1 must stay
what lenet_ref.pool1_exact defines: the maximum of the exact sums, rounded once.  What can go wrong on the device only: the quad
permutations (a lane that takes the wrong neighbour loses a maximum that sits at ONE position), the selection of the lane's own
filter, the addresses (an image that arrives through the queue and the staging path, a launch with fewer images than workgroups).
So the data puts every filter's maximum at every position of a window, and 258 images are one more round than the 256 persistent
workgroups take at once.  Images repeat a dozen distinct ones, so that all 258 are compared for the price of twelve references.

conv2 writes every pooled value as three bf16 pieces, split in pairs by v_cvt_pk_bf16_f32: the pieces must be lenet_ref.split3_bits
of the f32 they add up to.
"""
import numpy as np
import pytest

import lenet_ref
from gpd_amd import synth

N_FEW, N_QUEUE = 3, 258   # fewer images than workgroups; just more than the 256 persistent workgroups
SPECIAL = 5               # C = 15: the filter with one huge and one tiny weight


def _fixed_point(w, C):
    c1w = w["c1w"].reshape(20, C, 5, 5)
    Wi, s = np.zeros(c1w.shape, np.int64), np.zeros(20, np.int64)
    for f in range(20):
        mx = float(np.abs(c1w[f]).max())
        s[f] = 30 - int(np.frexp(mx)[1]) if mx > 0 else 0
        Wi[f] = np.rint(c1w[f].astype(np.float64) * 2.0 ** int(s[f])).astype(np.int64)
    return Wi, s


def _exact_sums(img_hwc, Wi):
    """[20][56][56] int64: the exact sums of W * x the kernel forms (digit planes + correction)"""
    return lenet_ref.conv_valid(np.transpose(img_hwc, (2, 0, 1)).astype(np.int64), Wi)


def _windows(S):
    """[20][56][56] -> [20][28][28][4]: position = 2 * (row in window) + (column in window)"""
    return S.reshape(20, 28, 2, 28, 2).transpose(0, 1, 3, 2, 4).reshape(20, 28, 28, 4)


def _weights(C):
    w = synth.lenet_weights(C, seed=11, trained_magnitude=True)
    if C == 15:
        # one filter whose sums differ by less than an f32 ulp inside a window: a huge weight on a constant plane, a tiny one
        # (W = 3 at the filter's fixed point) on a varying plane
        c1w = w["c1w"].reshape(20, C, 5, 5).copy()
        c1w[SPECIAL] = 0
        c1w[SPECIAL, 0, 0, 0] = 1.0
        c1w[SPECIAL, 1, 4, 4] = 3.0 * 2.0 ** -29
        w["c1w"] = c1w.ravel()
    return w


def _distinct_images(C, w):
    """a dozen images: mostly-zero random ones, the constants 0 / 128 / 255, one per quad position (C = 15: chosen for filter 0)"""
    rng = np.random.RandomState(200 + C)
    rnd = rng.randint(0, 256, (5, 60, 60, C)).astype(np.uint8)
    rnd[rng.rand(5, 60, 60, C) < 0.6] = 0
    if C == 15:
        rnd[1, :, :, 0] = 200   # the special filter's constant plane under its varying one
    const = [np.full((60, 60, C), v, np.uint8) for v in (255, 0, 128)]
    # period-2 images, one phase lit: every window of a filter's conv sees the same four sums, and the lit phase moves their
    # maximum from position to position
    Wi, _ = _fixed_point(w, C)
    T = np.array([[Wi[0][:, a::2, b::2].sum() for b in (0, 1)] for a in (0, 1)])   # filter 0's sum over the taps of a parity class
    a0, b0 = np.unravel_index(np.argmax(T), T.shape)
    phase = []
    for pos in range(4):
        py, px = (a0 + (pos >> 1)) % 2, (b0 + (pos & 1)) % 2
        im = np.zeros((60, 60, C), np.uint8)
        im[py::2, px::2] = 255
        phase.append(im)
    # the first three: a random one, a constant, a phase image (the launch with fewer images than workgroups)
    return [rnd[0], const[0], phase[0], rnd[1], const[1], phase[1], rnd[2], const[2], phase[2], rnd[3], phase[3], rnd[4]], phase


_CACHE = {}


def _case(C):
    """weights, the distinct images and their references: built once per channel count, shared by the tests, never modified"""
    if C not in _CACHE:
        w = _weights(C)
        distinct, phase = _distinct_images(C, w)
        ref = [lenet_ref.pool1_exact(im, w, C) for im in distinct]
        for a in distinct + ref:
            a.setflags(write=False)
        _CACHE[C] = (w, distinct, phase, ref)
    return _CACHE[C]


def _batch(distinct, n):
    idx = np.arange(n) % len(distinct)
    return np.stack([distinct[i] for i in idx]), idx


def test_the_data_is_what_the_case_needs():
    """(on the CPU, before the device is trusted) C = 15, ReLU off, n = 258"""
    C = 15
    w, distinct, phase, _ = _case(C)
    Wi, s = _fixed_point(w, C)
    corr = 128 * Wi.reshape(20, -1).sum(axis=1)
    win = np.stack([_windows(_exact_sums(im, Wi)) for im in distinct])          # [image][20][28][28][4]
    top = win.max(axis=-1, keepdims=True)
    unique_max = ((win == top).sum(axis=-1) == 1)[..., None] & (win == top)      # the maximum sits at ONE position
    # every filter has its window maximum at each of the four positions somewhere
    seen = unique_max.any(axis=(0, 2, 3))                                        # [20][4]
    assert seen.all(), np.argwhere(~seen)
    # the phase images: filter 0's maximum at the chosen position of EVERY window
    for pos, im in enumerate(phase):
        k = [i for i, d in enumerate(distinct) if d is im][0]
        assert unique_max[k, 0, :, :, pos].all(), pos
    # a window with two distinct exact sums that round to the same float
    r = win.astype(np.float64).astype(np.float32)
    same = False
    for a in range(4):
        for b in range(a + 1, 4):
            same |= bool(((win[..., a] != win[..., b]) & (r[..., a] == r[..., b])).any())
    assert same
    # ... and one where they are the two largest: only a maximum taken AFTER a wrong rounding could tell them apart
    srt = np.sort(win, axis=-1)
    assert ((srt[..., 3] != srt[..., 2]) & (srt[..., 3].astype(np.float64).astype(np.float32) == srt[..., 2].astype(np.float64).astype(np.float32))).any()
    # a negative pooled value, and one that is exactly the correction alone (the constant image 128: every digit sum is zero)
    assert (top < 0).any()
    k128 = [i for i, d in enumerate(distinct) if (d == 128).all()][0]
    assert (top[k128][..., 0] == corr[:, None, None]).all()
    # all of the batch's 258 images are covered, and the two that come through the queue differ from their predecessors
    _, idx = _batch(distinct, N_QUEUE)
    assert set(idx) == set(range(len(distinct))) and idx[256] != idx[255] and idx[257] != idx[256]


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("C", [15, 12, 3, 1])
def test_pool1_bit_for_bit(C, relu):
    from gpd_amd import api
    w, distinct, _, ref = _case(C)
    ctx = api.Context(api.default_params(C))
    try:
        ctx.set_lenet_weights(w)
        ctx.set_lenet_mode(api.LENET_SPLIT)
        ctx.set_lenet_conv_relu(relu)
        for n in (N_FEW, N_QUEUE):
            img, idx = _batch(distinct, n)
            ctx.score(img)
            pool1 = ctx.lenet_debug(0, n).reshape(n, 28, 28, 20)
            want = np.stack([ref[i] for i in idx])
            if relu:
                want = np.maximum(want, np.float32(0))
            bad = np.argwhere(pool1.view(np.uint32) != want.view(np.uint32))
            assert len(bad) == 0, (n, len(bad), bad[:8])
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, N_QUEUE])
def test_x_pieces_are_the_split_of_their_sum(n):
    from gpd_amd import api
    C = 15
    w = synth.lenet_weights(C, seed=11, trained_magnitude=True)
    _, distinct, _, _ = _case(C)
    img, _ = _batch(distinct, n)
    ctx = api.Context(api.default_params(C))
    try:
        ctx.set_lenet_weights(w)
        ctx.set_lenet_mode(api.LENET_SPLIT)
        ctx.score(img)
        xs = ctx.lenet_debug(1, n)                                               # [3][n][7200] bf16 bit patterns
        flat = lenet_ref.bf16_to_f64(xs[0]) + lenet_ref.bf16_to_f64(xs[1]) + lenet_ref.bf16_to_f64(xs[2])
        f32 = flat.astype(np.float32)
        assert np.array_equal(f32.astype(np.float64), flat)                      # the sum is an f32
        assert np.abs(flat).max() > 0
        h, m, l = lenet_ref.split3_bits(f32)
        assert np.array_equal(xs[0], h) and np.array_equal(xs[1], m) and np.array_equal(xs[2], l)
    finally:
        ctx.close()
