"""Plain numpy restatements of the split LeNet path's stages, shared by the GPU tests of that path
(test_gpu_lenet_fast.py, test_gpu_lenet_limits.py).  Float64 / int64 throughout: no GPU, no oracle."""
import numpy as np


def bf16_to_f64(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def split3_bits(x):
    """The three round-to-nearest-even bf16 pieces (bit patterns) of every f32 of x: h, then the residual's, then its residual's"""
    def rne(a):
        b = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
        return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)

    def val(u):
        return (u.astype(np.uint32) << 16).view(np.float32)
    x = np.ascontiguousarray(x, np.float32)
    h = rne(x)
    r1 = (x - val(h)).astype(np.float32)
    m = rne(r1)
    return h, m, rne((r1 - val(m)).astype(np.float32))


def has_subnormal_piece(x):
    """Whether a bf16 piece of some f32 of x is subnormal (the pieces then no longer reassemble the f32: the split path's
    exactness argument, test_lenet_fast_tables.py test_pieces_reassemble_exactly, does not cover such inputs)"""
    return any((((p & 0x7F80) == 0) & ((p & 0x7F) != 0)).any() for p in split3_bits(x))


def conv_valid(x, w):
    """x [C, H, W], w [F, C, 5, 5] -> [F, H - 4, W - 4] in int64 (x int64) or float64"""
    F = w.shape[0]
    H, W = x.shape[1] - 4, x.shape[2] - 4
    out = np.zeros((F, H, W), np.int64 if x.dtype == np.int64 else np.float64)
    for ky in range(5):
        for kx in range(5):
            out += np.einsum("fc,chw->fhw", w[:, :, ky, kx], x[:, ky:ky + H, kx:kx + W])
    return out


def pool(h):
    F, H, W = h.shape
    return h.reshape(F, H // 2, 2, W // 2, 2).max(axis=(2, 4))


def pool1_exact(img_hwc, w, C):
    """conv1 + pool1 as the split path defines it: integer dot products with round(w 2^s), one rounding, + bias"""
    c1w = w["c1w"].reshape(20, C, 5, 5)
    x = np.transpose(img_hwc, (2, 0, 1)).astype(np.int64)
    out = np.zeros((20, 28, 28), np.float32)
    for f in range(20):
        mx = float(np.abs(c1w[f]).max())
        s = 30 - int(np.frexp(mx)[1]) if mx > 0 else 0
        Wi = np.rint(c1w[f].astype(np.float64) * 2.0 ** s).astype(np.int64)[None]
        h = pool(conv_valid(x, Wi))[0]
        out[f] = np.ldexp(h.astype(np.float32), -s).astype(np.float32) + w["c1b"][f]
    return np.transpose(out, (1, 2, 0))  # [row][column][filter]
