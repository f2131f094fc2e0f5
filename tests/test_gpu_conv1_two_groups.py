"""conv1's two frames on the device (gpd_amd/csrc/lenet_fast.hip, conv1_i8_body), bit for bit at the image counts where the
persistent launch can go wrong.

Sixteen-byte pixels (C = 15) and the narrow geometries (C <= 4) run two 256-thread workgroups per CU: G = 2 x CUs workgroups
take image blockIdx.x first and then whatever the launch's counter hands out, and every image goes from global memory straight
into the pixel-major LDS copy.  Twelve channels keep one 512-thread workgroup per CU and the raw copy.  What can go wrong there
and nowhere else: a workgroup that takes the wrong image, takes one twice or leaves one out (the ticket arithmetic against the
grid of the launch, the counter between launches), and the rows a partial last round of the turn leaves unwritten.  So every
image differs from every other (seeded random bytes, about half of them zero), and the counts sit around the first ticket round:

    1, 2             fewer images than one CU's two workgroups
    G - 1, G, G + 1  the first round complete or not; a workgroup whose first ticket is already past the end
    2 G + 7          several rounds per workgroup with a ragged last one

pool1 must be what lenet_ref.pool1_exact defines (integer dot products with round(w 2^s), ONE rounding to f32, the maximum,
ldexp, + bias), restated here on torch's float64 conv2d: every product and every partial sum is an integer below 2^53, so the
float64 sums are exact in any order.  test_the_reference_is_pool1_exact ties the restatement to the model on the CPU.
"""
import ctypes

import numpy as np
import pytest

import lenet_ref
from gpd_amd import synth

_CACHE = {}


def _reference(C, images):
    """[n][28][28][20] f32: lenet_ref.pool1_exact for a batch, on float64 conv2d (exact: see the module's text)"""
    import torch
    import torch.nn.functional as F
    w = synth.lenet_weights(C, seed=11, trained_magnitude=True)
    c1w = w["c1w"].reshape(20, C, 5, 5)
    Wi, s = np.zeros(c1w.shape, np.float64), np.zeros(20, np.int64)
    for f in range(20):
        mx = float(np.abs(c1w[f]).max())
        s[f] = 30 - int(np.frexp(mx)[1]) if mx > 0 else 0
        Wi[f] = np.rint(c1w[f].astype(np.float64) * 2.0 ** int(s[f]))
    out = np.zeros((len(images), 28, 28, 20), np.float32)
    Wt = torch.from_numpy(Wi)
    for a in range(0, len(images), 64):
        x = torch.from_numpy(np.ascontiguousarray(np.transpose(images[a:a + 64], (0, 3, 1, 2)))).to(torch.float64)
        S = F.max_pool2d(F.conv2d(x, Wt), 2).numpy()                       # [n][20][28][28], exact integers
        v = np.ldexp(S.astype(np.float32), -s[None, :, None, None]).astype(np.float32) + w["c1b"][None, :, None, None]
        out[a:a + 64] = np.transpose(v, (0, 2, 3, 1))
    return w, out


def _case(C, n_max):
    """weights, n_max distinct images and their references: built once per channel count (for the largest count any test asks
    for: the smaller batches are prefixes), shared by the tests, never modified"""
    if C not in _CACHE or len(_CACHE[C][1]) < n_max:
        rng = np.random.RandomState(700 + C)
        img = rng.randint(0, 256, (n_max, 60, 60, C)).astype(np.uint8)
        img[rng.rand(n_max, 60, 60, C) < 0.5] = 0
        w, ref = _reference(C, img)
        img.setflags(write=False)
        ref.setflags(write=False)
        _CACHE[C] = (w, img, ref)
    return _CACHE[C]


def _groups():
    """G: the workgroups of a two-group launch that has images enough = 2 x the CU count, which the library takes from
    hipGetDeviceProperties and this asks the same runtime for (through the library's own handle)"""
    from gpd_amd import api
    cus = ctypes.c_int(0)
    rc = api.lib().hipDeviceGetAttribute(ctypes.byref(cus), 63, 0)   # hipDeviceAttributeMultiprocessorCount, device 0
    assert rc == 0 and cus.value > 0, (rc, cus.value)
    return 2 * cus.value


def _check(ctx, img, ref, n, relu):
    ctx.score(img[:n])
    pool1 = ctx.lenet_debug(0, n).reshape(n, 28, 28, 20)
    want = np.maximum(ref[:n], np.float32(0)) if relu else ref[:n]
    bad = np.argwhere(pool1.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (n, len(bad), sorted(set(bad[:, 0]))[:8], bad[:4])


def _context(C, w, relu):
    from gpd_amd import api
    ctx = api.Context(api.default_params(C))
    ctx.set_lenet_weights(w)
    ctx.set_lenet_mode(api.LENET_SPLIT)
    ctx.set_lenet_conv_relu(relu)
    return ctx


@pytest.mark.parametrize("C", [15, 12, 3])
def test_the_reference_is_pool1_exact(C):
    """(on the CPU) the float64 restatement against the model of tests/test_gpu_conv1_pool.py, and the images all differ"""
    rng = np.random.RandomState(5)
    img = rng.randint(0, 256, (3, 60, 60, C)).astype(np.uint8)
    img[rng.rand(3, 60, 60, C) < 0.5] = 0
    w, ref = _reference(C, img)
    for k in range(3):
        assert np.array_equal(ref[k].view(np.uint32), lenet_ref.pool1_exact(img[k], w, C).view(np.uint32))
    assert len({im.tobytes() for im in img}) == 3
    assert (ref < 0).any() and (ref > 0).any()      # the ReLU cases clamp something and keep something


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("count", ["1", "2", "G-1", "G", "G+1", "2G+7"])
def test_sixteen_byte_pixels(count, relu):
    G = _groups()
    n = {"1": 1, "2": 2, "G-1": G - 1, "G": G, "G+1": G + 1, "2G+7": 2 * G + 7}[count]
    w, img, ref = _case(15, 2 * G + 7)
    assert len({im.tobytes() for im in img[:n]}) == n
    ctx = _context(15, w, relu)
    try:
        _check(ctx, img, ref, n, relu)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("count", ["2", "G+1"])
def test_narrow_pixels(count):
    """C = 3: four-byte pixels in four shifted copies, in the two-group frame as well"""
    G = _groups()
    n = {"2": 2, "G+1": G + 1}[count]
    w, img, ref = _case(3, G + 1)
    ctx = _context(3, w, False)
    try:
        _check(ctx, img, ref, n, False)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_twelve_channels_keep_one_group_per_cu():
    """C = 12 does not fit the LDS twice: the old frame, a grid of min(n, CUs), the raw copy — beside the new launch arithmetic"""
    n = _groups() + 1
    w, img, ref = _case(12, n)
    ctx = _context(12, w, False)
    try:
        _check(ctx, img, ref, n, False)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_two_lists_back_to_back():
    """the launch's image counter between launches: a long list, a short one, the long one again, on one context"""
    G = _groups()
    w, img, ref = _case(15, 2 * G + 7)
    ctx = _context(15, w, False)
    try:
        _check(ctx, img, ref, G + 5, False)
        _check(ctx, img[7:], ref[7:], 3, False)
        _check(ctx, img[3:], ref[3:], G + 5, False)
    finally:
        ctx.close()
