"""GPD_LENET_NET_SPLIT without a device: gpd_hip_bf16_split3 — the definition of the pieces the split kernels of the
shape-general route multiply, and of their weight tables — against a numpy restatement (integer rounding on the f32 bits), the
refusals of gpd_hip_set_lenet_net_mode that need no context, the api constants, and the host mirror's cfg key."""
import os

import numpy as np

from gpd_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bf16_bits(x):
    """Round to nearest even of finite f32 to bf16, on the bits"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def _bf16_value(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def _split3(x):
    x = np.ascontiguousarray(x, np.float32)
    h = _bf16_bits(x)
    r1 = x - _bf16_value(h)  # exact in f32
    m = _bf16_bits(r1)
    r2 = r1 - _bf16_value(m)
    return h, m, _bf16_bits(r2)


def _values():
    rng = np.random.RandomState(2)
    seeded = (rng.choice([-1.0, 1.0], 20000) * rng.uniform(1, 2, 20000) * np.exp2(rng.randint(-100, 100, 20000))).astype(np.float32)
    pows = np.exp2(np.arange(-100, 101)).astype(np.float32)
    # ties of the first rounding (the 16 dropped bits are 0x8000, kept lsb even and odd), of the second, and neighbours
    bits = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3F800080, 0x3F800180, 0x3F8000C0, 0x3F7FFFFF, 0x3F800001,
                     0x40490FDB, 0x717FFFFF], np.uint32).view(np.float32)
    return np.concatenate([seeded, np.zeros(3, np.float32), pows, -pows, bits, -bits, np.arange(256, dtype=np.float32)])


def test_bf16_split3_is_the_numpy_restatement_and_sums_exactly():
    x = _values()
    assert np.isfinite(x).all() and ((x == 0) | (np.abs(x) >= np.float32(2.0 ** -100))).all()
    h, m, l = api.bf16_split3(x)
    wh, wm, wl = _split3(x)
    assert np.array_equal(h, wh) and np.array_equal(m, wm) and np.array_equal(l, wl)
    hv, mv, lv = (_bf16_value(p).astype(np.float64) for p in (h, m, l))
    assert np.array_equal(hv + mv + lv, x.astype(np.float64))
    nz = mv != 0
    assert nz.sum() > 10000 and (np.abs(mv[nz]) <= 2.0 ** -8 * np.abs(hv[nz])).all()
    nz = lv != 0
    assert nz.sum() > 5000 and (np.abs(lv[nz]) <= 2.0 ** -8 * np.abs(mv[nz])).all()
    # a u8 is one piece
    small = np.arange(256, dtype=np.float32)
    h, m, l = api.bf16_split3(small)
    assert np.array_equal(_bf16_value(h), small) and not m.any() and not l.any()
    # shapes are kept, an empty array is legal
    h, m, l = api.bf16_split3(np.ones((3, 5), np.float32))
    assert h.shape == m.shape == l.shape == (3, 5)
    assert api.bf16_split3(np.zeros(0, np.float32))[0].shape == (0,)


def test_bf16_split3_refuses_null_pointers():
    L = api.lib()
    assert L.gpd_hip_bf16_split3(None, 4, None, None, None) == -1
    assert b"gpd_hip_bf16_split3: bad argument" in L.gpd_hip_last_error()
    assert L.gpd_hip_bf16_split3(None, 0, None, None, None) == 0


def test_net_mode_refuses_a_null_context_and_the_constants_exist():
    L = api.lib()
    assert (api.LENET_NET_CHAIN, api.LENET_NET_SPLIT) == (0, 1)
    assert "gpd_hip_set_lenet_net_mode" in api.EXPORTS and "gpd_hip_bf16_split3" in api.EXPORTS
    for mode in (0, 1, 7):
        assert L.gpd_hip_set_lenet_net_mode(None, mode) == -1
        assert L.gpd_hip_last_error() == b"gpd_hip_set_lenet_net_mode: bad argument"
    import inspect
    assert "net_mode" in inspect.signature(api.Context.set_lenet_net).parameters
    assert "net_mode" in inspect.signature(api.Trainer.install).parameters
    with open(os.path.join(ROOT, "include", "gpd_hip.h")) as f:
        header = f.read()
    assert "#define GPD_LENET_NET_CHAIN 0" in header and "#define GPD_LENET_NET_SPLIT 1" in header


def test_host_mirror_knows_the_cfg_key():
    """Without a device the CLI cannot get as far as a classifier (test_gpu_lenet_net_split.py runs it with the key set); what can
    be held here is that the mirror was built with the key and the entry it drives"""
    cli = os.path.join(ROOT, "gpd_amd", "host", "detect_grasps")
    assert os.path.exists(cli)
    blobs = b""
    host = os.path.join(ROOT, "gpd_amd", "host")
    for f in os.listdir(host):
        p = os.path.join(host, f)
        if os.path.isfile(p) and (f == "detect_grasps" or f.endswith(".so")):
            with open(p, "rb") as fh:
                blobs += fh.read()
    assert b"hip_lenet_net_mode" in blobs
