"""Independent numpy statement of the seeded shadow jitter (include/gpd_hip.h, gpd_hip_set_shadow_jitter): the mix, the draw
g of a voxel, and pyref.grasp_image with the shadow points moved by it.  Integer arithmetic modulo 2^64 and exact double
operations only, so it equals the host model and the kernels bit for bit.  Shares no code with gpd_amd/csrc/jitter_model.h."""
import math

import numpy as np

import pyref

U64 = np.uint64
VOXEL = 0.003


def mix(z):
    """splitmix64's step on uint64 arrays (numpy wraps modulo 2^64)."""
    z = np.asarray(z, U64)
    with np.errstate(over="ignore"):
        z = z + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def draws(seed, voxels):
    """g of every voxel [n, 3] (int32) under `seed`: the twelve 16-bit fields of k1, k2, k3 summed, centred, / 65536."""
    v = np.asarray(voxels, np.int32).reshape(-1, 3)
    u = v.view(np.uint32).astype(U64)  # two's complement, zero-extended
    k0 = mix(U64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ (u[:, 0] | (u[:, 1] << U64(32))))
    k1 = mix(k0 ^ u[:, 2])
    k2 = mix(k1)
    k3 = mix(k2)
    S = np.zeros(len(v), np.int64)
    for k in (k1, k2, k3):
        for sh in (0, 16, 32, 48):
            S += ((k >> U64(sh)) & U64(0xFFFF)).astype(np.int64)
    return (S - 393210).astype(np.float64) * (1.0 / 65536.0)


def shadow_points(voxels, seed):
    """p_a = (double)v_a * 0.003 + (g * 0.003) * 0.3, the same draw on all three coordinates (hand_set.cpp:197-199) -> f64 [n, 3]"""
    v = np.asarray(voxels, np.int32).reshape(-1, 3)
    g = draws(seed, v)
    return v.astype(np.float64) * VOXEL + ((g * VOXEL) * 0.3)[:, None]


def lattice_points(voxels):
    return np.asarray(voxels, np.int32).reshape(-1, 3).astype(np.float64) * VOXEL


def in_box(P, hand, pts):
    """findPointsInUnitImage on f64 points [n, 3], vectorised with pyref._to_unit's operand order -> bool [n]"""
    F = np.asarray(hand["frame"], np.float64).reshape(3, 3)
    c = np.asarray(pts, np.float64).reshape(-1, 3) - np.asarray(hand["sample"], np.float64)
    t = [F[0, r] * c[:, 0] + F[1, r] * c[:, 1] + F[2, r] * c[:, 2] for r in range(3)]
    b, ce, half = float(hand["bottom"]), float(hand["center"]), P.volume_width / 2.0
    return ((t[0] > b) & (t[0] < b + P.volume_depth) & (t[1] > ce - half) & (t[1] < ce + half)
            & (t[2] > -1.0 * P.volume_height) & (t[2] < P.volume_height))


def shadow_voxels(pts, view_point, rng, shadow_length=0.10):
    """pyref.shadow_voxels with the point arithmetic done on arrays (the same IEEE operations per element, the draws in the
    same order from the same pyref.Lcg) -> lexicographically sorted unique voxel list."""
    pts = np.asarray(pts, np.float64)
    center = np.zeros(3)
    for p in pts:
        center = center + p
    center = center / float(len(pts))
    vec = center - np.asarray(view_point, np.float64)
    vec = shadow_length * vec / math.sqrt(vec[0] * vec[0] + vec[1] * vec[1] + vec[2] * vec[2])
    n_sh = int(math.floor(shadow_length / 0.003))
    t = np.array([float(rng.next()) for _ in range(len(pts) * n_sh)], np.float64) * (1.0 / 32767.0)
    q = (np.repeat(pts, n_sh, axis=0) + t[:, None] * vec[None, :]) * (1.0 / 0.003)
    return sorted(set(map(tuple, np.trunc(q).astype(np.int64).tolist())))


def shadow_voxels_cameras(pts, cam_rows, view_points, rng, shadow_length=0.10):
    """pyref.shadow_voxels_cameras over shadow_voxels above: the intersection is taken on voxels."""
    cam_rows = np.asarray(cam_rows)
    sets = [set(shadow_voxels(pts, view_points[c], rng, shadow_length)) if cam_rows[c].sum() >= 1 else set()
            for c in range(cam_rows.shape[0])]
    allv = sets[0]
    for c in range(1, cam_rows.shape[0]):
        if cam_rows[c].sum() >= 1:
            allv = allv & sets[c]
    return sorted(allv)


def grasp_image_jitter(P, hand, xyz, normals, nbr_idx, shadow_vox, seed):
    """pyref.grasp_image with the shadow points moved off the lattice.  The voxels stay in their lexicographic order: that is
    the order in which their points enter a pixel's running mean (image_strategy.cpp:202-210)."""
    C = P.image_num_channels
    assert C == 15
    img = pyref.grasp_image(P, hand, xyz, normals, nbr_idx, [])  # the twelve channels that hold no shadow
    vox = np.asarray(shadow_vox, np.int64).reshape(-1, 3).astype(np.int32)
    sp = shadow_points(vox, seed)
    # only a point near the box can pass pyref._to_unit's test: the others are dropped here, by a margin of a millimetre
    # in every hand coordinate against rounding errors of 1e-15 (the loop below is per point, in Python)
    F = np.asarray(hand["frame"], np.float64).reshape(3, 3)
    t = (sp - np.asarray(hand["sample"], np.float64)) @ F
    b, ce, half, m = float(hand["bottom"]), float(hand["center"]), P.volume_width / 2.0, 1e-3
    near = ((t[:, 0] > b - m) & (t[:, 0] < b + P.volume_depth + m) & (t[:, 1] > ce - half - m) & (t[:, 1] < ce + half + m)
            & (np.abs(t[:, 2]) < P.volume_height + m))
    _, su = pyref._to_unit(F, np.asarray(hand["sample"], np.float64), b, ce, sp[near], P)
    perm = [(0, 1, 2), (2, 1, 0), (2, 0, 1)]
    for pr in range(3):
        a, bb, d = perm[pr]
        sc = pyref._cells(su[:, a], su[:, bb]) if len(su) else []
        img[..., pr * 5 + 4] = pyref._shadow_image(su[:, d] if len(su) else [], sc)
    return img
