"""The draws of the importance-sampling driver (gpd_amd/csrc/sis_model.h), restated in pure Python for the tests.

Round r has two xorshift64 streams (pyref_sample.stream), seeds in uint32 arithmetic: Gaussian seed + 1000003 * (2r), uniform
seed + 1000003 * (2r + 1).  A Gaussian proposal is 7 draws (idx_raw, three Box-Muller offsets of two draws each), a uniform
proposal one (pos_raw).  Floats are Python floats (IEEE doubles, no contraction); log / sqrt / cos are the math module's, which
calls the same libm as the library on the machine the tests run on."""
import itertools
import math

import numpy as np

from pyref_sample import stream

PROPOSAL_DTYPE = np.dtype([("idx_raw", "<u8"), ("off", "<f8", (3,))], align=False)


def stream_seed(seed, rnd, kind):
    return (seed + 1000003 * (2 * rnd + kind)) & 0xFFFFFFFF


def rand_normal(g, sigma):
    u1 = (float(next(g) >> 11) + 1.0) * (1.0 / 9007199254740993.0)
    u2 = float(next(g) >> 11) * (1.0 / 9007199254740992.0)
    return sigma * math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)


def uniforms(seed, rnd, first, count):
    """The 53-bit uniforms (u1, u2) behind the three offsets of Gaussian proposals first .. first + count -> f64 [count, 3, 2]."""
    g = stream(stream_seed(seed, rnd, 0))
    out = np.zeros((count, 3, 2))
    for i, d in enumerate(itertools.islice(g, 7 * first, 7 * (first + count))):
        k = i % 7
        if k == 0:
            continue
        out[i // 7, (k - 1) // 2, (k - 1) % 2] = ((float(d >> 11) + 1.0) * (1.0 / 9007199254740993.0) if (k - 1) % 2 == 0
                                                   else float(d >> 11) * (1.0 / 9007199254740992.0))
    return out


def proposals(seed, rnd, kind, first, count, sigma=0.02):
    g = stream(stream_seed(seed, rnd, kind))
    if kind == 1:
        return np.array(list(itertools.islice(g, first, first + count)), np.uint64).reshape(-1)
    for _ in range(7 * first):
        next(g)
    out = np.zeros(count, PROPOSAL_DTYPE)
    for i in range(count):
        out["idx_raw"][i] = next(g)
        for r in range(3):
            out["off"][i, r] = rand_normal(g, sigma)
    return out


def d2(x, c):
    dx, dy, dz = x[0] - c[0], x[1] - c[1], x[2] - c[2]
    return (dx * dx + dy * dy) + dz * dz


def select(centres, gauss, uniform, uniform_list, cloud_xyz, workspace, method, num_gauss, num_rand, state=None):
    """The selection rule over one block of each stream, written as the reference's sequential loops
    (sequential_importance_sampling.cpp:189-270); `state`: what an earlier call on the round's previous blocks returned."""
    cen = [[float(v) for v in c] for c in np.asarray(centres, np.float64).reshape(-1, 3)]
    L = len(cen)
    xyz = np.asarray(cloud_xyz, np.float32).reshape(-1, 3)
    ws = [float(v) for v in workspace]
    n = num_gauss + num_rand
    samples = np.zeros((n, 3)) if state is None else np.array(state["samples"], np.float64).reshape(n, 3).copy()
    acc = [0, 0] if state is None else [int(v) for v in state["accepted"]]
    used = [0, 0] if state is None else [int(v) for v in state["consumed"]]
    for p in gauss:
        if acc[0] >= num_gauss:
            break
        idx = int(p["idx_raw"]) % L
        x = [cen[idx][r] + float(p["off"][r]) for r in range(3)]
        ok = True
        if method == 1:
            own = d2(x, cen[idx])
            ok = own <= min(d2(x, c) for c in cen)
        if ok:
            samples[acc[0]] = x
            acc[0] += 1
        used[0] += 1
    for raw in uniform:
        if acc[1] >= num_rand:
            break
        pt = int(uniform_list[int(raw) % len(uniform_list)]) if uniform_list is not None and len(uniform_list) else int(raw) % len(xyz)
        s = [float(xyz[pt, r]) for r in range(3)]
        if ws[0] <= s[0] <= ws[1] and ws[2] <= s[1] <= ws[3] and ws[4] <= s[2] <= ws[5]:
            samples[num_gauss + acc[1]] = s
            acc[1] += 1
        used[1] += 1
    return dict(samples=samples, accepted=np.array(acc, np.int32), consumed=np.array(used, np.int32),
                shortfall=(num_gauss - acc[0]) + (num_rand - acc[1]))


def num_rand_samples(prob_rand_samples, num_samples):
    return int(prob_rand_samples * num_samples)


def draw_round(seed, rnd, centres, uniform_list, cloud_xyz, workspace, method, num_samples, prob_rand_samples, sigma, block=256,
               max_blocks=4096):
    """A whole round: blocks of both streams until the list is full -> the dict of select()."""
    num_rand = num_rand_samples(prob_rand_samples, num_samples)
    num_gauss = num_samples - num_rand
    st, first = None, [0, 0]
    for _ in range(max_blocks):
        need_g = st is None or st["accepted"][0] < num_gauss
        need_u = st is None or st["accepted"][1] < num_rand
        g = proposals(seed, rnd, 0, first[0], block if need_g else 0, sigma)
        u = proposals(seed, rnd, 1, first[1], block if need_u else 0)
        first = [first[0] + len(g), first[1] + len(u)]
        st = select(centres, g, u, uniform_list, cloud_xyz, workspace, method, num_gauss, num_rand, st)
        if st["shortfall"] == 0:
            return st
    raise RuntimeError("the draw of round %d does not fill its list" % rnd)
