"""conv1's tile epilogue (gpd_amd/csrc/lenet_fast.hip, conv1_i8_body) rests on two facts that need no GPU to check:

  * the pool may run on the four ROUNDED values: (float) max_i (S_i + corr) == max_i (float)(S_i + corr) for integer sums,
    bit for bit, and the rounded values are never NaN and never -0 (the kernel takes its maxima with a bare v_max_f32);
  * the correction 128 * sum(W) may START the digit sums (corr = c3 * 2^24 + c0 through the first MFMA's C operand): the kernel
    recombines hi = (D3 << 8) + D2 and lo = (D1 << 8) + D0 in 32 bits, so |hi|, |lo| < 2^31 must hold for every image.
"""
import glob
import os

import numpy as np
import pytest

from gpd_amd import synth
from test_lenet_fast_tables import _tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f32(s):
    """int64 (below 2^53 in magnitude) -> f32, one rounding to nearest even: what v_cvt_f32_f64 of the exact f64 gives"""
    s = np.asarray(s, np.int64)
    assert (np.abs(s) < 2 ** 53).all()
    return s.astype(np.float64).astype(np.float32)


def _adversarial_windows():
    w = []
    # distinct sums that round to the same f32: above 2^24 the spacing is 2^(e - 23)
    for e in (25, 30, 40, 45):
        ulp = 1 << (e - 23)
        base = (1 << e) + 5 * ulp
        w.append([base, base + 1, base - 1, base + ulp // 2 - 1])
        w.append([-base, -base + 1, -base - 1, -base - ulp // 2 + 1])
    # sums just either side of a rounding boundary (the tie between two floats), and the tie itself (goes to the even one)
    for e in (24, 25, 31, 44):
        ulp = 1 << (e - 23)
        for k in (0, 1, 2, 3):
            tie = (1 << e) + k * ulp + ulp // 2
            w.append([tie - 1, tie, tie + 1, tie - ulp])
            w.append([tie + 1, tie - 1, tie - 1, tie - 1])
            w.append([-(tie - 1), -tie, -(tie + 1), -(tie + ulp)])
            w.append([tie, tie, tie - 1, tie - 1])
    # all values equal; all negative; a total of exactly 0 as the maximum, and as a non-maximum
    for v in (0, 1, -1, (1 << 24) + 1, -(1 << 40) - 12345, (1 << 45) + 3):
        w.append([v] * 4)
    w.append([-1, -2, -(1 << 30), -(1 << 45)])
    w.append([-(1 << 24) - 1, -(1 << 24) - 2, -(1 << 24) - 3, -(1 << 24) - 1])
    w.append([0, -1, -(1 << 33), -7])
    w.append([-5, 0, 0, -5])
    w.append([0, 5, -5, 1])
    win = np.array(w, np.int64)
    # ... every rotation of every window: the maximum at each of the four positions
    return np.concatenate([np.roll(win, r, axis=1) for r in range(4)])


def test_round_then_max_is_max_then_round():
    win = _adversarial_windows()
    rng = np.random.RandomState(3)
    # random windows of near neighbours at every magnitude the kernel can meet (|S + corr| < 2^47)
    centre = (rng.randint(-2 ** 46, 2 ** 46, (4000, 1), dtype=np.int64) >> rng.randint(0, 46, (4000, 1))).astype(np.int64)
    win = np.concatenate([win, centre + rng.randint(-3, 4, (4000, 4))])
    rounded = _f32(win)                       # the kernel: round each, ...
    pooled = rounded.max(axis=1)              # ... then the quad's maximum
    ref = _f32(win.max(axis=1))               # the definition (lenet_ref.pool1_exact): the maximum of the exact sums, rounded once
    assert np.array_equal(pooled.view(np.uint32), ref.view(np.uint32))
    # a bare v_max_f32 is only the maximum for operands that are neither NaN nor -0
    assert not np.isnan(rounded).any()
    assert not (np.signbit(rounded) & (rounded == 0)).any()
    # the cases are what they claim to be
    distinct_same = [(len(set(r)) > 1) and len(set(_f32(r).tolist())) < len(set(r)) for r in win[:200].tolist()]
    assert sum(distinct_same) >= 16
    assert (win.max(axis=1) < 0).any() and (win.max(axis=1) == 0).any() and (win == win[:, :1]).all(axis=1).any()


def _digits(W):
    """four balanced base-256 digits of int64 W, least significant first, as lenet_fast_conv1_tables cuts them"""
    out, v = [], W.copy()
    for _ in range(4):
        d = ((v + 128) & 255) - 128
        out.append(d)
        v = (v - d) >> 8
    assert (v == 0).all()
    return out


def _start_values(corr):
    c = corr.astype(np.int64)
    assert (c == corr).all()
    c0 = ((c + (1 << 23)) & 0xFFFFFF) - (1 << 23)
    c3 = (c - c0) >> 24
    assert (c3 * (1 << 24) + c0 == c).all()
    return c0, c3


def _check_bounds(channels, c1w, images=()):
    """|hi|, |lo| < 2^31 for ANY image (every tap at |x - 128| = 128 with the worst sign), and exactly for the given constant images"""
    w = synth.lenet_weights(channels, seed=1)
    w["c1w"] = np.ascontiguousarray(c1w, np.float32).ravel()
    _, corr, shift, _ = _tables(channels, w)   # (its return code is the host's own assertion of the same bounds)
    K = channels * 25
    c1 = w["c1w"].reshape(20, K).astype(np.float64)
    W = np.rint(c1 * 2.0 ** shift[:, None].astype(np.float64)).astype(np.int64)
    assert (np.abs(W) <= 2 ** 30).all()
    assert np.array_equal(corr, 128.0 * W.sum(axis=1))
    d = _digits(W)
    assert np.abs(d[3]).max() <= 64
    c0, c3 = _start_values(corr)
    mag = [np.abs(x).sum(axis=1) for x in d]
    hi = (128 * mag[3] + np.abs(c3)) * 256 + 128 * mag[2]
    lo = 128 * mag[1] * 256 + 128 * mag[0] + np.abs(c0)
    assert (hi < 2 ** 31).all() and (lo < 2 ** 31).all(), (hi.max(), lo.max())
    for x in images:   # a constant image: every tap sees x - 128
        D = [x_d.sum(axis=1) * (x - 128) for x_d in d]
        hi_x = ((D[3] + c3) << 8) + D[2]
        lo_x = (D[1] << 8) + D[0] + c0
        assert (np.abs(hi_x) < 2 ** 31).all() and (np.abs(lo_x) < 2 ** 31).all()
        assert np.array_equal(hi_x * 65536 + lo_x, W.sum(axis=1) * x)   # the exact sum of W * x, as pool1_exact defines it
    return float(hi.max()) / 2 ** 31, float(lo.max()) / 2 ** 31


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "lenet*_params.npz"))), ids=os.path.basename)
def test_start_value_bounds_of_the_golden_tables(path):
    p = np.load(path)
    channels = p["c1w"].size // 500
    _check_bounds(channels, p["c1w"], images=(0, 128, 255))


@pytest.mark.parametrize("channels", [16, 15, 12, 3, 1])
@pytest.mark.parametrize("sign", ["plus", "minus", "alternating"])
def test_start_value_bounds_of_a_hostile_set(channels, sign):
    """every weight of a filter at the largest magnitude a filter's fixed point allows (|W| = 2^30 - 64 and exactly 2^30 / 2),
    all of one sign (the correction is at its largest) or alternating (the digit sums are, the correction is not)"""
    K = channels * 25
    big = np.float32(np.nextafter(np.float32(2.0), np.float32(0.0)))     # 24 ones: W = 2^30 - 64
    c1w = np.zeros((20, K), np.float32)
    for f in range(20):
        mag = big * np.float32(2.0) ** (f - 10) if f % 2 == 0 else np.float32(2.0) ** (f - 10)
        s = {"plus": np.ones(K), "minus": -np.ones(K), "alternating": (-1.0) ** np.arange(K)}[sign]
        c1w[f] = (mag * s).astype(np.float32)
    hi, lo = _check_bounds(channels, c1w, images=(0, 255, 1, 127, 128))
    assert hi < 0.8 and lo < 0.8   # (the proof in lenet_fast.hip: below 1.70e9 = 0.79 * 2^31 at 16 channels)
