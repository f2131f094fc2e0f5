"""ctypes binding of libgpd_hip.so (include/gpd_hip.h) — the product path.

There is no CPU fallback: if the HIP library is missing or a call fails, this
raises.  The Python layer only marshals numpy arrays into the C-ABI.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GPD_HIP_LIB: another build of the same library (A/B timing of a kernel change on one GPU box)
LIB_PATH = os.environ.get("GPD_HIP_LIB") or os.path.join(_HERE, "libgpd_hip.so")
_LIB = None

# numpy mirror of `gpd_hand` (include/gpd_hip.h)
HAND_DTYPE = np.dtype([
    ("sample", "<f8", (3,)), ("frame", "<f8", (9,)), ("position", "<f8", (3,)),
    ("top", "<f8"), ("bottom", "<f8"), ("center", "<f8"), ("grasp_width", "<f8"),
    ("score", "<f4"), ("finger_placement_index", "<i4"), ("set_index", "<i4"), ("slot", "<i4"),
    ("valid", "u1"), ("half_antipodal", "u1"), ("full_antipodal", "u1"), ("pad_", "u1", (5,)),
], align=False)


class Params(C.Structure):
    """Mirror of `gpd_params` (include/gpd_hip.h)."""
    _fields_ = [
        ("finger_width", C.c_double), ("hand_outer_diameter", C.c_double), ("hand_depth", C.c_double),
        ("hand_height", C.c_double), ("init_bite", C.c_double), ("volume_width", C.c_double),
        ("volume_depth", C.c_double), ("volume_height", C.c_double), ("nn_radius_frames", C.c_double),
        ("friction_coeff", C.c_double), ("min_aperture", C.c_double), ("max_aperture", C.c_double),
        ("workspace_grasps", C.c_double * 6), ("image_size", C.c_int32), ("image_num_channels", C.c_int32),
        ("num_orientations", C.c_int32), ("num_finger_placements", C.c_int32), ("num_hand_axes", C.c_int32),
        ("hand_axes", C.c_int32 * 3), ("deepen_hand", C.c_int32), ("min_viable", C.c_int32),
        ("filter_approach_direction", C.c_int32), ("reserved_", C.c_int32), ("direction", C.c_double * 3), ("thresh_rad", C.c_double),
    ]


class DetectJob(C.Structure):
    """Mirror of `gpd_detect_job` (include/gpd_hip.h)."""
    _fields_ = [
        ("xyz", C.c_void_p), ("normals", C.c_void_p), ("cam_source", C.c_void_p), ("view_points", C.c_void_p),
        ("sample_indices", C.c_void_p), ("hands", C.c_void_p),
        ("num_points", C.c_int32), ("num_cams", C.c_int32), ("num_samples", C.c_int32), ("num_selected", C.c_int32),
        ("hands_capacity", C.c_int32), ("num_sets", C.c_int32), ("num_candidates", C.c_int32), ("num_hands", C.c_int32),
        ("status", C.c_int32), ("stage_ms", C.c_float * 3), ("host_ms", C.c_float * 5), ("allocs", C.c_int32),
        ("reserved_", C.c_int32), ("lcg_base", C.c_uint64), ("lcg_draws", C.c_uint64),
        ("raw", C.c_int32), ("voxel_size", C.c_float), ("workspace", C.c_void_p), ("normals_radius", C.c_double), ("sample_xyz", C.c_void_p),
        ("num_points_processed", C.c_int32), ("num_samples_processed", C.c_int32),
        ("refine_normals_k", C.c_int32), ("sample_above_plane", C.c_int32), ("num_draws", C.c_int32), ("sample_seed", C.c_uint32),
        ("samples_out", C.c_void_p),
        ("refine_passes", C.c_int32), ("refine_num_nan", C.c_int32), ("plane_num_above", C.c_int32), ("plane_iterations", C.c_int32),
        ("preprocess_ms", C.c_float * 4),
        ("outlier_mean_k", C.c_int32), ("num_outliers", C.c_int32), ("outlier_stddev_mult", C.c_double), ("outlier_ms", C.c_float),
        ("reserved2_", C.c_int32),
    ]


class LabelViewJob(C.Structure):
    """Mirror of `gpd_label_view_job` (include/gpd_hip.h)."""
    _fields_ = [
        ("sample_indices", C.c_void_p), ("samples_per_round", C.c_int32), ("max_rounds", C.c_int32),
        ("min_positives", C.c_int32), ("max_grasps_per_view", C.c_int32),
        ("images", C.c_void_p), ("labels", C.c_void_p), ("hands", C.c_void_p), ("src_index", C.c_void_p), ("capacity", C.c_int32),
        ("all_labels", C.c_void_p), ("all_labels_capacity", C.c_int32), ("round_counts", C.c_void_p),
        ("rounds_run", C.c_int32), ("num_candidates", C.c_int32), ("num_positives", C.c_int32), ("num_out", C.c_int32),
        ("num_positives_out", C.c_int32), ("gt_neighbourhoods", C.c_int32), ("d2h_bytes", C.c_int64), ("stage_ms", C.c_float * 4),
    ]


class SisJob(C.Structure):
    """Mirror of `gpd_sis_job` (include/gpd_hip.h)."""
    _fields_ = [
        ("sample_indices", C.c_void_p), ("num_init_samples", C.c_int32), ("num_iterations", C.c_int32), ("num_samples", C.c_int32),
        ("sampling_method", C.c_int32), ("prob_rand_samples", C.c_double), ("sigma", C.c_double), ("min_score", C.c_double),
        ("workspace", C.c_double * 6), ("min_inliers", C.c_int32), ("remove_inliers", C.c_int32), ("seed", C.c_uint32),
        ("proposal_block", C.c_int32), ("hands", C.c_void_p), ("capacity", C.c_int32), ("num_hands", C.c_int32),
        ("rounds_run", C.c_int32), ("num_sets", C.c_int32), ("num_candidates", C.c_int32), ("centres_capacity", C.c_int32),
        ("samples_out", C.c_void_p), ("centres_out", C.c_void_p), ("round_counts", C.c_void_p), ("d2h_bytes", C.c_int64),
        ("stage_ms", C.c_float * 4),
    ]


# numpy mirror of `gpd_sis_proposal` (include/gpd_hip.h)
SIS_PROPOSAL_DTYPE = np.dtype([("idx_raw", "<u8"), ("off", "<f8", (3,))], align=False)


class TrainParams(C.Structure):
    """Mirror of `gpd_train_params` (include/gpd_hip.h)."""
    _fields_ = [("channels", C.c_int32), ("max_batch", C.c_int32), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double), ("weight_decay", C.c_double), ("input_scale", C.c_double)]


class TrainRecipe(C.Structure):
    """Mirror of `gpd_train_recipe` (include/gpd_hip.h)."""
    _fields_ = [("network", C.c_int32), ("solver", C.c_int32), ("momentum", C.c_double), ("lr_policy", C.c_int32), ("stepsize", C.c_int32),
                ("gamma", C.c_double), ("power", C.c_double), ("lr_mult", C.c_double * 8), ("decay_mult", C.c_double * 8)]


# gpd_train_recipe's enums, and the solver file's base_lr (it belongs in TrainParams.lr)
NET_TORCH, NET_CAFFE = 0, 1
SOLVER_ADAM, SOLVER_SGD = 0, 1
LR_FIXED, LR_STEP, LR_EXP, LR_INV = 0, 1, 2, 3
CAFFE_BASE_LR = 0.01


class GpdHipError(RuntimeError):
    pass


# gpd_hip_set_lenet_mode (include/gpd_hip.h)
LENET_SPLIT, LENET_F32_CHAIN = 0, 1
LENET_NET_CHAIN, LENET_NET_SPLIT = 0, 1  # gpd_hip_set_lenet_net_mode: the arithmetic of the shape-general route


def sample_positions(n, num_draws, seed=0, with_repetition=False):
    """gpd_hip_sample_positions: the positions Cloud::subsample(num_draws) draws from a list of n entries (host only) -> i32."""
    out = np.zeros(max(min(int(num_draws), int(n)), 1), np.int32)
    k = C.c_int(0)
    rc = lib().gpd_hip_sample_positions(int(n), int(num_draws), int(seed) & 0xFFFFFFFF, int(bool(with_repetition)), _ptr(out), C.byref(k))
    if rc != 0:
        raise GpdHipError("libgpd_hip error %d: %s" % (rc, lib().gpd_hip_last_error().decode()))
    return out[: k.value].copy()


def balance_view(labels, max_grasps_per_view):
    """gpd_hip_balance_view: DataGenerator::balanceInstances over a view's accumulated labels (host only) -> the indices of the
    kept candidates, i32: the first `end` positives, then the first `end` negatives, end = min(P, N, max_grasps_per_view // 2)."""
    lab = np.ascontiguousarray(labels, np.uint8).reshape(-1)
    out = np.zeros(max(2 * (max(int(max_grasps_per_view), 0) // 2), 1), np.int32)
    n, npos = C.c_int(0), C.c_int(0)
    rc = lib().gpd_hip_balance_view(_ptr(lab), len(lab), int(max_grasps_per_view), _ptr(out), C.byref(n), C.byref(npos))
    if rc != 0:
        raise GpdHipError("libgpd_hip error %d: %s" % (rc, lib().gpd_hip_last_error().decode()))
    assert n.value == 2 * npos.value
    return out[: n.value].copy()


def shuffle_orders(seed, sizes):
    """gpd_hip_shuffle_orders: the orders in which generate_data stores instance sets of the given sizes, one seeded stream
    running through them in order (host only) -> list of i32 arrays; order[k] = the instance that ends up at position k."""
    sizes = np.ascontiguousarray(sizes, np.int32).reshape(-1)
    out = np.zeros(max(int(sizes.sum()), 1), np.int32)
    rc = lib().gpd_hip_shuffle_orders(int(seed) & 0xFFFFFFFF, _ptr(sizes), len(sizes), _ptr(out))
    if rc != 0:
        raise GpdHipError("libgpd_hip error %d: %s" % (rc, lib().gpd_hip_last_error().decode()))
    edges = np.concatenate([[0], np.cumsum(sizes)])
    return [out[a:b].copy() for a, b in zip(edges[:-1], edges[1:])]


def sis_proposals(seed, round, kind, first, count, sigma=0.02):
    """gpd_hip_sis_proposals: proposals first .. first + count of a stream of importance-sampling round `round` (host only) ->
    kind 0: SIS_PROPOSAL_DTYPE [count] (idx_raw, three Gaussian offsets); kind 1: u64 [count] (pos_raw)."""
    out = np.zeros(max(int(count), 1), SIS_PROPOSAL_DTYPE if int(kind) == 0 else np.uint64)
    rc = lib().gpd_hip_sis_proposals(int(seed) & 0xFFFFFFFF, int(round), int(kind), int(first), int(count), float(sigma), _ptr(out))
    if rc != 0:
        raise GpdHipError("libgpd_hip error %d: %s" % (rc, lib().gpd_hip_last_error().decode()))
    return out[: int(count)].copy()


def sis_select(centres, gauss, uniform, uniform_list, cloud_xyz, workspace, sampling_method, num_gauss, num_rand, state=None):
    """gpd_hip_sis_select: the selection rule of an importance-sampling round over one block of each stream (host only).
    state: the dict an earlier call on the round's previous blocks returned (None: the round's first blocks).
    -> dict: samples f64 [num_gauss + num_rand, 3], accepted i32 [2], consumed i32 [2] (Gaussian, uniform), shortfall."""
    cen = np.ascontiguousarray(centres, np.float64).reshape(-1, 3)
    g = np.ascontiguousarray(gauss, SIS_PROPOSAL_DTYPE).reshape(-1)
    u = np.ascontiguousarray(uniform, np.uint64).reshape(-1)
    lst = None if uniform_list is None else np.ascontiguousarray(uniform_list, np.int32).reshape(-1)
    xyz = np.ascontiguousarray(cloud_xyz, np.float32).reshape(-1, 3)
    ws = np.ascontiguousarray(workspace, np.float64).reshape(6)
    n = int(num_gauss) + int(num_rand)
    if state is None:
        samples, acc, used = np.zeros((max(n, 1), 3), np.float64), np.zeros(2, np.int32), np.zeros(2, np.int32)
    else:
        samples = np.zeros((max(n, 1), 3), np.float64)
        samples[:n] = state["samples"]
        acc, used = state["accepted"].astype(np.int32).copy(), state["consumed"].astype(np.int32).copy()
    short = C.c_int(0)
    rc = lib().gpd_hip_sis_select(_ptr(cen) if len(cen) else None, len(cen), _ptr(g) if len(g) else None, len(g),
                                  _ptr(u) if len(u) else None, len(u), _ptr(lst) if lst is not None and len(lst) else None,
                                  0 if lst is None else len(lst), _ptr(xyz) if len(xyz) else None, len(xyz), _ptr(ws),
                                  int(sampling_method), int(num_gauss), int(num_rand), _ptr(samples), _ptr(acc), _ptr(used), C.byref(short))
    if rc != 0:
        raise GpdHipError("libgpd_hip error %d: %s" % (rc, lib().gpd_hip_last_error().decode()))
    return dict(samples=samples[:n].copy(), accepted=acc, consumed=used, shortfall=int(short.value))


class ImageModel(C.Structure):
    """Mirror of `gpd_image_model` (include/gpd_hip.h)."""
    _fields_ = [("window_class", C.c_int32), ("set_sd", C.c_int32), ("set_sr", C.c_int32), ("num_shadow", C.c_int32),
                ("stride_a", C.c_uint32), ("stride_c", C.c_uint32), ("true_div", C.c_int32), ("reserved_", C.c_int32),
                ("thr", (C.c_double * 61) * 3)]


def image_model(params, shadow_jitter=None):
    """gpd_hip_image_model: what the image stage derives from the geometry in `params` (host only) -> dict: window_class,
    set_sd, set_sr, num_shadow, stride_a, stride_c, true_div and thr f64 [3, 61].  With `shadow_jitter` (0 or 1)
    gpd_hip_image_model_jitter: the windows of that setting of Context.set_shadow_jitter."""
    m = ImageModel()
    if shadow_jitter is None:
        rc = lib().gpd_hip_image_model(C.byref(params), C.byref(m))
    else:
        rc = lib().gpd_hip_image_model_jitter(C.byref(params), int(shadow_jitter), C.byref(m))
    if rc != 0:
        raise GpdHipError("libgpd_hip error %d: %s" % (rc, lib().gpd_hip_last_error().decode()))
    out = {k: int(getattr(m, k)) for k in ("window_class", "set_sd", "set_sr", "num_shadow", "stride_a", "stride_c", "true_div")}
    out["thr"] = np.array(m.thr, np.float64).reshape(3, 61)
    return out


def shadow_jitter_model(seed, voxels):
    """gpd_hip_shadow_jitter_model: the draw g of every voxel in `voxels` (int32 [n, 3]) under `seed` (host only) -> f64 [n]."""
    v = np.ascontiguousarray(voxels, np.int32)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError("voxels must be [n, 3]")
    g = np.empty(v.shape[0], np.float64)
    rc = lib().gpd_hip_shadow_jitter_model(int(seed) & 0xFFFFFFFFFFFFFFFF, v.ctypes.data, v.shape[0], g.ctypes.data)
    if rc != 0:
        raise GpdHipError("libgpd_hip error %d: %s" % (rc, lib().gpd_hip_last_error().decode()))
    return g


TORCH_KEYS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")


def torch_state_arrays(state):
    """The eight tensors of pytorch/network.py::Net out of a state_dict-like mapping -> {key: contiguous f32 array} in torch
    layout.  Values are numpy arrays or anything with .detach().cpu().numpy() (torch is not imported here); a `module.` prefix
    on the keys (a model wrapped in nn.DataParallel, as pytorch/train_net3.py may save it) is stripped."""
    plain = {}
    for k, v in state.items():
        k = str(k)
        plain[k[len("module."):] if k.startswith("module.") else k] = v
    out = {}
    for k in TORCH_KEYS:
        if k not in plain:
            raise KeyError("state dict has no %r (keys: %s)" % (k, sorted(plain)))
        v = plain[k]
        if hasattr(v, "detach"):
            v = v.detach().cpu().numpy()
        out[k] = np.ascontiguousarray(v, np.float32)
    return out


def lenet_from_torch(state, channels, input_scale=1.0 / 256):
    """gpd_hip_lenet_from_torch: a state dict of the reference's PyTorch network (pytorch/network.py::Net, trained on
    image * input_scale, hdf5_dataset.py:17) -> the c1w .. f2b dict set_lenet_weights takes.  Host only.  The network also
    needs Context.set_lenet_conv_relu(True); Context.set_lenet_torch does both."""
    t = torch_state_arrays(state)
    channels = int(channels)
    sizes = {"conv1.weight": 20 * channels * 25, "conv1.bias": 20, "conv2.weight": 50 * 500, "conv2.bias": 50,
             "fc1.weight": 500 * 7200, "fc1.bias": 500, "fc2.weight": 2 * 500, "fc2.bias": 2}
    for k, n in sizes.items():
        if t[k].size != n:
            raise ValueError("%s has %d elements, %d expected for %d channels" % (k, t[k].size, n, channels))
    c1w, f1w, f2w = np.zeros(20 * channels * 25, np.float32), np.zeros(7200 * 500, np.float32), np.zeros(1000, np.float32)
    L = lib()
    rc = L.gpd_hip_lenet_from_torch(channels, float(input_scale), _ptr(t["conv1.weight"]), _ptr(t["fc1.weight"]), _ptr(t["fc2.weight"]),
                                    _ptr(c1w), _ptr(f1w), _ptr(f2w))
    if rc != 0:
        raise GpdHipError("libgpd_hip error %d: %s" % (rc, L.gpd_hip_last_error().decode()))
    # conv2 [50][20][5][5] is the reference's [50][500] already, and the biases are biases
    return dict(c1w=c1w, c1b=t["conv1.bias"].ravel().copy(), c2w=t["conv2.weight"].ravel().copy(), c2b=t["conv2.bias"].ravel().copy(),
                f1w=f1w, f1b=t["fc1.bias"].ravel().copy(), f2w=f2w, f2b=t["fc2.bias"].ravel().copy())


class LenetShape(C.Structure):
    """gpd_lenet_shape (include/gpd_hip.h): C -> conv1_out -> conv2_out -> fc1_out [-> fc2_out] -> 2; fc2_out = 0: no third
    dense layer (pytorch/network.py::Net), > 0: NetCCFFF."""
    _fields_ = [("channels", C.c_int32), ("conv1_out", C.c_int32), ("conv2_out", C.c_int32), ("fc1_out", C.c_int32), ("fc2_out", C.c_int32)]

    def as_tuple(self):
        return (self.channels, self.conv1_out, self.conv2_out, self.fc1_out, self.fc2_out)

    def __repr__(self):
        return "LenetShape(channels=%d, conv1_out=%d, conv2_out=%d, fc1_out=%d, fc2_out=%d)" % self.as_tuple()


TORCH_NET_KEYS = TORCH_KEYS + ("fc3.weight", "fc3.bias")


def lenet_shape_check(shape):
    """gpd_hip_lenet_shape_check -> True when the shape is within the limits of the general route."""
    return lib().gpd_hip_lenet_shape_check(C.byref(shape)) == 0


def torch_net_arrays(state):
    """A state dict of pytorch/network.py::Net or ::NetCCFFF of any widths -> (LenetShape, [8 or 10 contiguous f32 arrays in
    torch layout, conv1.weight .. fc2.bias (.. fc3.bias)]).  The shape is read off the tensors; fc3.* keys select NetCCFFF.
    Values and the `module.` prefix as in torch_state_arrays.  ValueError when the tensors do not fit one another."""
    plain = {}
    for k, v in state.items():
        k = str(k)
        plain[k[len("module."):] if k.startswith("module.") else k] = v
    has3 = "fc3.weight" in plain or "fc3.bias" in plain
    arrs = []
    for k in (TORCH_NET_KEYS if has3 else TORCH_KEYS):
        if k not in plain:
            raise KeyError("state dict has no %r (keys: %s)" % (k, sorted(plain)))
        v = plain[k]
        if hasattr(v, "detach"):
            v = v.detach().cpu().numpy()
        arrs.append(np.ascontiguousarray(v, np.float32))
    c1, c2, f1, f2 = arrs[0], arrs[2], arrs[4], arrs[6]
    if c1.ndim != 4 or c1.shape[2:] != (5, 5) or c2.ndim != 4 or c2.shape[2:] != (5, 5) or f1.ndim != 2 or f2.ndim != 2:
        raise ValueError("conv weights must be [out][in][5][5] and dense weights [out][in]: got %s"
                         % [tuple(a.shape) for a in (c1, c2, f1, f2)])
    F1, Cn = c1.shape[:2]
    F2, H1 = c2.shape[0], f1.shape[0]
    want = [(F1, Cn, 5, 5), (F1,), (F2, F1, 5, 5), (F2,), (H1, F2 * 144), (H1,)]
    if has3:
        H2 = f2.shape[0]
        want += [(H2, H1), (H2,), (2, H2), (2,)]
    else:
        H2 = 0
        want += [(2, H1), (2,)]
    for k, a, w in zip(TORCH_NET_KEYS, arrs, want):
        if tuple(a.shape) != w:
            raise ValueError("%s has shape %s, %s expected from the other tensors" % (k, tuple(a.shape), w))
    return LenetShape(int(Cn), int(F1), int(F2), int(H1), int(H2)), arrs


def _pointer_table(arrs):
    t = (C.c_void_p * 10)()
    for i, a in enumerate(arrs):
        t[i] = a.ctypes.data
    return t


def bf16_split3(x):
    """gpd_hip_bf16_split3: the three bf16 pieces (uint16 bit patterns h, m, l, shaped like x) of float32 values, as the split
    kernels and their weight tables make them.  Host only."""
    x = np.ascontiguousarray(x, np.float32)
    h, m, l = (np.zeros(x.shape, np.uint16) for _ in range(3))
    if lib().gpd_hip_bf16_split3(_ptr(x), x.size, _ptr(h), _ptr(m), _ptr(l)) != 0:
        raise GpdHipError(lib().gpd_hip_last_error().decode())
    return h, m, l


def lenet_net_from_torch(state, input_scale=1.0 / 256):
    """gpd_hip_lenet_net_from_torch: a state dict of Net / NetCCFFF (see torch_net_arrays) -> (LenetShape, the 8 or 10 tensors
    in the layouts gpd_hip_set_lenet_net takes).  Host only."""
    shape, arrs = torch_net_arrays(state)
    outs = [np.zeros(a.size, np.float32) for a in arrs]
    L = lib()
    rc = L.gpd_hip_lenet_net_from_torch(C.byref(shape), float(input_scale), _pointer_table(arrs), _pointer_table(outs))
    if rc != 0:
        raise GpdHipError("libgpd_hip error %d: %s" % (rc, L.gpd_hip_last_error().decode()))
    return shape, outs


def bind_host_thread(device):
    """gpd_hip_bind_host_thread: the calling thread onto the CPUs of the device's NUMA node -> (node or -1, cpus)."""
    n = C.c_int(0)
    node = lib().gpd_hip_bind_host_thread(int(device), C.byref(n))
    return int(node), int(n.value)


EXPORTS = ["gpd_hip_default_params", "gpd_hip_create", "gpd_hip_destroy", "gpd_hip_last_error",
           "gpd_hip_set_lenet_weights", "gpd_hip_score", "gpd_hip_upload_cloud", "gpd_hip_search",
           "gpd_hip_images", "gpd_hip_detect", "gpd_hip_last_stage_ms", "gpd_hip_replay", "gpd_hip_replay_times", "gpd_hip_last_images_stats", "gpd_hip_estimate_normals",
           "gpd_hip_search_samples", "gpd_hip_detect_samples", "gpd_hip_reevaluate", "gpd_hip_replay_kernel_ms", "gpd_hip_last_centre_chains",
           "gpd_hip_detect_select", "gpd_hip_detect_batch", "gpd_hip_detect_batch_multi", "gpd_hip_conv1_stats", "gpd_hip_last_fallbacks", "gpd_hip_preprocess_cloud", "gpd_hip_find_clusters", "gpd_hip_reserve", "gpd_hip_bind_host_thread",
           "gpd_hip_set_lenet_mode", "gpd_hip_lenet_debug", "gpd_hip_lenet_fast_tables", "gpd_hip_detect_sharded",
           "gpd_hip_sample_above_plane", "gpd_hip_last_image_routes", "gpd_hip_last_normals_routes", "gpd_hip_refine_normals", "gpd_hip_sample_positions",
           "gpd_hip_remove_statistical_outliers",
           "gpd_hip_set_lenet_conv_relu", "gpd_hip_lenet_from_torch",
           "gpd_hip_lenet_shape_check", "gpd_hip_lenet_net_from_torch", "gpd_hip_set_lenet_net", "gpd_hip_lenet_net_debug",
           "gpd_hip_lenet_net_info", "gpd_hip_set_lenet_net_mode", "gpd_hip_bf16_split3",
           "gpd_hip_upload_ground_truth", "gpd_hip_label_view", "gpd_hip_balance_view", "gpd_hip_sizeof_label_view_job",
           "gpd_hip_shuffle_orders", "gpd_hip_sis_proposals", "gpd_hip_sis_select", "gpd_hip_detect_sis", "gpd_hip_sizeof_sis_job",
           "gpd_hip_image_model", "gpd_hip_image_model_jitter", "gpd_hip_set_shadow_jitter", "gpd_hip_shadow_jitter_model",
           "gpd_hip_given_check", "gpd_hip_images_given", "gpd_hip_score_given",
           "gpd_hip_train_default_params", "gpd_hip_train_create", "gpd_hip_train_destroy", "gpd_hip_train_init_state",
           "gpd_hip_train_set_state", "gpd_hip_train_get_state", "gpd_hip_train_set_data", "gpd_hip_train_steps",
           "gpd_hip_train_gradients", "gpd_hip_train_apply", "gpd_hip_train_eval", "gpd_hip_train_step_timed",
           "gpd_hip_train_kernel_name", "gpd_hip_sizeof_train_recipe", "gpd_hip_train_default_recipe", "gpd_hip_train_create_recipe",
           "gpd_hip_train_init_xavier", "gpd_hip_train_learning_rate", "gpd_hip_train_get_solver_state",
           "gpd_hip_train_set_solver_state", "gpd_hip_train_kernel_name_of",
           "gpd_hip_train_reserve", "gpd_hip_train_count", "gpd_hip_train_append_data", "gpd_hip_train_get_data",
           "gpd_hip_train_reorder", "gpd_hip_train_append_view",
           "gpd_hip_train_group_mean", "gpd_hip_train_group_slices", "gpd_hip_train_group_schedule", "gpd_hip_train_group_create",
           "gpd_hip_train_group_destroy", "gpd_hip_train_group_broadcast", "gpd_hip_train_group_steps", "gpd_hip_train_group_verify",
           "gpd_hip_train_group_last_bytes",
           "gpd_hip_train_create_net", "gpd_hip_train_shape", "gpd_hip_train_net_set_state", "gpd_hip_train_net_get_state",
           "gpd_hip_train_net_gradients", "gpd_hip_train_net_apply", "gpd_hip_train_net_get_solver_state",
           "gpd_hip_train_net_set_solver_state", "gpd_hip_train_net_sizes", "gpd_hip_train_net_init_state",
           "gpd_hip_train_net_init_xavier"]


def build(prof=True):
    """Compile libgpd_hip.so for gfx950 (hipcc cross-compiles without a GPU) and, with `prof`, the profiling build
    libgpd_hip_prof.so (needs the roctx headers; the release library does not)."""
    subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(_HERE, "csrc")])
    if prof:
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(_HERE, "csrc"), "prof"])


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise GpdHipError("libgpd_hip.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                              "there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.gpd_hip_last_error.restype = C.c_char_p
        L.gpd_hip_create.argtypes = [C.c_int, C.POINTER(Params), C.POINTER(C.c_void_p)]
        L.gpd_hip_destroy.argtypes = [C.c_void_p]
        L.gpd_hip_destroy.restype = None
        L.gpd_hip_set_lenet_weights.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8
        L.gpd_hip_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.gpd_hip_upload_cloud.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.gpd_hip_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.gpd_hip_search_samples.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.gpd_hip_detect_samples.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.gpd_hip_reevaluate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.gpd_hip_images.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        L.gpd_hip_detect.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.gpd_hip_detect_select.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                            C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.gpd_hip_detect_batch.argtypes = [C.c_void_p, C.POINTER(DetectJob), C.c_int]
        L.gpd_hip_detect_batch_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(DetectJob), C.c_int]
        L.gpd_hip_detect_sharded.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(DetectJob)]
        L.gpd_hip_last_fallbacks.argtypes = [C.c_void_p, C.c_void_p]
        L.gpd_hip_last_image_routes.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.gpd_hip_last_normals_routes.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.gpd_hip_last_centre_chains.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        L.gpd_hip_last_stage_ms.argtypes = [C.c_void_p, C.c_void_p]
        L.gpd_hip_replay.argtypes = [C.c_void_p, C.c_int]
        L.gpd_hip_estimate_normals.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
        L.gpd_hip_sample_above_plane.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_double, C.c_int, C.c_void_p, C.POINTER(C.c_int),
                                                 C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.gpd_hip_refine_normals.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.POINTER(C.c_int), C.c_void_p,
                                             C.POINTER(C.c_int), C.c_void_p]
        L.gpd_hip_remove_statistical_outliers.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.POINTER(C.c_int), C.c_void_p,
                                                          C.c_void_p, C.c_void_p]
        L.gpd_hip_sample_positions.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.gpd_hip_find_clusters.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(C.c_int)]
        L.gpd_hip_preprocess_cloud.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)]
        L.gpd_hip_last_images_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.gpd_hip_replay_kernel_ms.argtypes = [C.c_void_p, C.c_void_p]
        L.gpd_hip_conv1_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.gpd_hip_reserve.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.gpd_hip_bind_host_thread.argtypes = [C.c_int, C.POINTER(C.c_int)]
        L.gpd_hip_set_lenet_mode.argtypes = [C.c_void_p, C.c_int]
        L.gpd_hip_set_lenet_conv_relu.argtypes = [C.c_void_p, C.c_int]
        L.gpd_hip_lenet_from_torch.argtypes = [C.c_int, C.c_double] + [C.c_void_p] * 6
        L.gpd_hip_lenet_debug.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.gpd_hip_lenet_shape_check.argtypes = [C.POINTER(LenetShape)]
        L.gpd_hip_lenet_net_from_torch.argtypes = [C.POINTER(LenetShape), C.c_double, C.c_void_p, C.c_void_p]
        L.gpd_hip_set_lenet_net.argtypes = [C.c_void_p, C.POINTER(LenetShape), C.c_void_p]
        L.gpd_hip_lenet_net_debug.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.gpd_hip_lenet_net_info.argtypes = [C.c_void_p, C.c_void_p]
        L.gpd_hip_set_lenet_net_mode.argtypes = [C.c_void_p, C.c_int]
        L.gpd_hip_bf16_split3.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gpd_hip_replay_times.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
        L.gpd_hip_upload_ground_truth.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.gpd_hip_label_view.argtypes = [C.c_void_p, C.POINTER(LabelViewJob)]
        L.gpd_hip_balance_view.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.gpd_hip_shuffle_orders.argtypes = [C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]
        L.gpd_hip_sis_proposals.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_double, C.c_void_p]
        L.gpd_hip_sis_select.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        L.gpd_hip_detect_sis.argtypes = [C.c_void_p, C.POINTER(SisJob)]
        L.gpd_hip_image_model.argtypes = [C.POINTER(Params), C.POINTER(ImageModel)]
        L.gpd_hip_image_model_jitter.argtypes = [C.POINTER(Params), C.c_int, C.POINTER(ImageModel)]
        L.gpd_hip_set_shadow_jitter.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
        L.gpd_hip_shadow_jitter_model.argtypes = [C.c_uint64, C.c_void_p, C.c_int, C.c_void_p]
        L.gpd_hip_given_check.argtypes = [C.POINTER(Params), C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.gpd_hip_images_given.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                           C.POINTER(C.c_uint64)]
        L.gpd_hip_score_given.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                          C.POINTER(C.c_uint64)]
        L.gpd_hip_train_default_params.argtypes = [C.POINTER(TrainParams)]
        L.gpd_hip_train_default_params.restype = None
        L.gpd_hip_train_create.argtypes = [C.c_void_p, C.POINTER(TrainParams), C.POINTER(C.c_void_p)]
        L.gpd_hip_train_destroy.argtypes = [C.c_void_p]
        L.gpd_hip_train_destroy.restype = None
        L.gpd_hip_train_init_state.argtypes = [C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]
        L.gpd_hip_train_set_state.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.gpd_hip_train_get_state.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.gpd_hip_train_set_data.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.gpd_hip_train_steps.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.gpd_hip_train_gradients.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_float)]
        L.gpd_hip_train_apply.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.gpd_hip_train_eval.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.gpd_hip_train_step_timed.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.gpd_hip_train_kernel_name.argtypes = [C.c_int]
        L.gpd_hip_train_kernel_name.restype = C.c_char_p
        L.gpd_hip_train_default_recipe.argtypes = [C.POINTER(TrainRecipe), C.c_int]
        L.gpd_hip_train_create_recipe.argtypes = [C.c_void_p, C.POINTER(TrainParams), C.POINTER(TrainRecipe), C.POINTER(C.c_void_p)]
        L.gpd_hip_train_init_xavier.argtypes = [C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]
        L.gpd_hip_train_learning_rate.argtypes = [C.POINTER(TrainRecipe), C.c_double, C.c_longlong, C.POINTER(C.c_float)]
        L.gpd_hip_train_get_solver_state.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)]
        L.gpd_hip_train_set_solver_state.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_longlong]
        L.gpd_hip_train_kernel_name_of.argtypes = [C.c_void_p, C.c_int]
        L.gpd_hip_train_kernel_name_of.restype = C.c_char_p
        L.gpd_hip_train_reserve.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.gpd_hip_train_count.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.gpd_hip_train_append_data.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.gpd_hip_train_get_data.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.gpd_hip_train_reorder.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.gpd_hip_train_append_view.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(LabelViewJob)]
        L.gpd_hip_train_group_mean.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_size_t, C.c_void_p]
        L.gpd_hip_train_group_slices.argtypes = [C.c_size_t, C.c_int, C.c_void_p]
        L.gpd_hip_train_group_schedule.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.gpd_hip_train_group_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]
        L.gpd_hip_train_group_destroy.argtypes = [C.c_void_p]
        L.gpd_hip_train_group_destroy.restype = None
        L.gpd_hip_train_group_broadcast.argtypes = [C.c_void_p, C.c_int]
        L.gpd_hip_train_group_steps.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.gpd_hip_train_group_verify.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        L.gpd_hip_train_group_last_bytes.argtypes = [C.c_void_p, C.c_void_p]
        L.gpd_hip_train_create_net.argtypes = [C.c_void_p, C.POINTER(TrainParams), C.POINTER(TrainRecipe), C.POINTER(LenetShape),
                                               C.POINTER(C.c_void_p)]
        L.gpd_hip_train_shape.argtypes = [C.c_void_p, C.POINTER(LenetShape)]
        L.gpd_hip_train_net_set_state.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.gpd_hip_train_net_get_state.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.gpd_hip_train_net_gradients.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_float)]
        L.gpd_hip_train_net_apply.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.gpd_hip_train_net_get_solver_state.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)]
        L.gpd_hip_train_net_set_solver_state.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_longlong]
        L.gpd_hip_train_net_sizes.argtypes = [C.POINTER(LenetShape), C.c_void_p]
        L.gpd_hip_train_net_init_state.argtypes = [C.POINTER(LenetShape), C.c_uint32, C.POINTER(C.c_void_p)]
        L.gpd_hip_train_net_init_xavier.argtypes = [C.POINTER(LenetShape), C.c_uint32, C.POINTER(C.c_void_p)]
        assert L.gpd_hip_sizeof_train_recipe() == C.sizeof(TrainRecipe)
        assert L.gpd_hip_sizeof_label_view_job() == C.sizeof(LabelViewJob)
        assert L.gpd_hip_sizeof_sis_job() == C.sizeof(SisJob)
        _LIB = L
    return _LIB


def given_check(params, hands):
    """gpd_hip_given_check: may these hand sets [num_sets, slots] be handed to Context.images_given / score_given?  Host only.
    -> None, or (set, slot, reason) of the first record outside the domain."""
    hands = np.ascontiguousarray(hands, HAND_DTYPE)
    slots = params.num_hand_axes * params.num_orientations
    if hands.ndim != 2 or hands.shape[1] != slots:
        raise ValueError("hands must be [num_sets, %d] records, set-major" % slots)
    bs, bj = C.c_int(-1), C.c_int(-1)
    rc = lib().gpd_hip_given_check(C.byref(params), _ptr(hands), hands.shape[0], C.byref(bs), C.byref(bj))
    if rc == 0:
        return None
    return int(bs.value), int(bj.value), lib().gpd_hip_last_error().decode()


def default_params(channels=15):
    p = Params()
    lib().gpd_hip_default_params(C.byref(p))
    p.image_num_channels = channels
    return p


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Context:
    """One gpd_hip_ctx: owns the device copy of the cloud, the LeNet weights and all scratch."""

    def __init__(self, params=None, device=0):
        self.params = params if params is not None else default_params()
        self._h = C.c_void_p()
        self._check(lib().gpd_hip_create(int(device), C.byref(self.params), C.byref(self._h)))
        self.n_slots = self.params.num_hand_axes * self.params.num_orientations

    def _check(self, rc):
        if rc != 0:
            raise GpdHipError("libgpd_hip error %d: %s" % (rc, lib().gpd_hip_last_error().decode()))

    def close(self):
        if self._h:
            lib().gpd_hip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_lenet_weights(self, w):
        arrs = [np.ascontiguousarray(w[k], np.float32) for k in ("c1w", "c1b", "c2w", "c2b", "f1w", "f1b", "f2w", "f2b")]
        ch = self.params.image_num_channels
        assert arrs[0].size == 20 * ch * 25, "conv1 weights do not match image_num_channels"
        self._check(lib().gpd_hip_set_lenet_weights(self._h, ch, *[_ptr(a) for a in arrs]))

    def set_lenet_mode(self, mode):
        """LENET_SPLIT (default: int8 / bf16 matrix pipes on exactly split operands) or LENET_F32_CHAIN (the oracle's
        k-ascending fmaf chains, bit-identical, 1/16 of the matrix rate)."""
        self._check(lib().gpd_hip_set_lenet_mode(self._h, int(mode)))

    def set_shadow_jitter(self, on, seed=0):
        """gpd_hip_set_shadow_jitter: the shadow points of every later image-making call leave the 3 mm lattice by a draw that is a
        pure function of (seed, voxel) — the reference's magnitude and arithmetic (hand_set.cpp:187-204), not its unseeded
        stream.  Off by default; without a shadow channel (1, 3, 12 channels) it changes nothing."""
        self._check(lib().gpd_hip_set_shadow_jitter(self._h, int(bool(on)), int(seed) & 0xFFFFFFFFFFFFFFFF))

    def set_lenet_conv_relu(self, on):
        """gpd_hip_set_lenet_conv_relu: a ReLU after conv1 and conv2 (the reference's PyTorch network) for every later scoring
        call of the context; off (default): the reference's Eigen / Caffe network.  Kept across set_lenet_weights."""
        self._check(lib().gpd_hip_set_lenet_conv_relu(self._h, int(bool(on))))

    def set_lenet_torch(self, state, input_scale=1.0 / 256):
        """A state dict of pytorch/network.py::Net (see lenet_from_torch) as the context's scoring network: weights + conv ReLUs."""
        self.set_lenet_weights(lenet_from_torch(state, self.params.image_num_channels, input_scale))
        self.set_lenet_conv_relu(True)

    def set_lenet_net(self, state, input_scale=1.0 / 256, conv_relu=True, net_mode=None):
        """A state dict of pytorch/network.py::Net or ::NetCCFFF of any widths within the limits (LenetShape) as the context's
        scoring network, on the shape-general route (exact f32 chains by default; set_lenet_mode is ignored by it,
        set_lenet_net_mode chooses its arithmetic — net_mode: that call as a convenience, None leaves the context's mode alone).
        set_lenet_weights / set_lenet_torch return the context to the stock route.  -> the LenetShape"""
        shape, arrs = lenet_net_from_torch(state, input_scale)
        self._lenet_shape = shape
        if net_mode is not None:
            self.set_lenet_net_mode(net_mode)
        self._check(lib().gpd_hip_set_lenet_net(self._h, C.byref(shape), _pointer_table(arrs)))
        self.set_lenet_conv_relu(conv_relu)
        return shape

    def set_lenet_net_mode(self, mode):
        """gpd_hip_set_lenet_net_mode: LENET_NET_CHAIN (default: the f32 chains, the bit-for-bit checker) or LENET_NET_SPLIT (the
        bf16 matrix pipe on exactly split operands, for throughput) for the shape-general route.  Context state: legal before or
        after set_lenet_net, kept across installs.  A change frees the route's scratch: install, set the mode, then reserve."""
        self._check(lib().gpd_hip_set_lenet_net_mode(self._h, int(mode)))

    def lenet_net_debug(self, which, n):
        """gpd_hip_lenet_net_debug: pool1 [n,F1,28,28] (0), pool2 [n,F2,12,12] (1), fc1 [n,H1] (2), fc2 [n,H2] (3) or the logits
        [n,2] (4) of the last scoring call, which must have taken the general route (GpdHipError otherwise)."""
        sh = getattr(self, "_lenet_shape", None)
        if sh is None:
            raise GpdHipError("lenet_net_debug: no network set by set_lenet_net")
        n = int(n)
        out = np.zeros({0: (n, sh.conv1_out, 28, 28), 1: (n, sh.conv2_out, 12, 12), 2: (n, sh.fc1_out), 3: (n, max(sh.fc2_out, 1)),
                        4: (n, 2)}[int(which)], np.float32)
        self._check(lib().gpd_hip_lenet_net_debug(self._h, int(which), n, _ptr(out)))
        return out

    def lenet_net_info(self):
        """gpd_hip_lenet_net_info -> dict(chunk_images, scratch_bytes_per_image, lds_bytes, macs_per_image)"""
        out = np.zeros(4, np.int64)
        self._check(lib().gpd_hip_lenet_net_info(self._h, _ptr(out)))
        return dict(chunk_images=int(out[0]), scratch_bytes_per_image=int(out[1]), lds_bytes=int(out[2]), macs_per_image=int(out[3]))

    def lenet_debug(self, which, n):
        """Test hook: pool1 (0), the flattened pool2 as bf16 planes (1) or ip1 transposed (2) of the last score() pass."""
        out = {0: np.zeros((n, 15680), np.float32), 1: np.zeros((3, n, 7200), np.uint16), 2: np.zeros((500, n), np.float32)}[which]
        self._check(lib().gpd_hip_lenet_debug(self._h, int(which), int(n), _ptr(out)))
        return out

    def score(self, images=None, n=None):
        """Classifier::classifyImages; images [n,60,60,C] u8, or None to score the device images."""
        if images is not None:
            images = np.ascontiguousarray(images, np.uint8)
            n = images.shape[0]
        out = np.zeros(n, np.float32)
        self._check(lib().gpd_hip_score(self._h, _ptr(images), n, _ptr(out)))
        return out

    def upload_cloud(self, xyz, normals, cam_source=None, view_points=None):
        xyz = np.ascontiguousarray(xyz, np.float32)
        normals = np.ascontiguousarray(normals, np.float32)
        P = len(xyz)
        cam = np.ones((1, P), np.int32) if cam_source is None else np.ascontiguousarray(cam_source, np.int32).reshape(-1, P)
        vp = np.zeros((1, 3)) if view_points is None else np.ascontiguousarray(view_points, np.float64).reshape(-1, 3)
        self._check(lib().gpd_hip_upload_cloud(self._h, _ptr(xyz), _ptr(normals), P, _ptr(cam), cam.shape[0], _ptr(vp)))
        self._num_points = P

    def upload_ground_truth(self, xyz, normals):
        """gpd_hip_upload_ground_truth: the ground-truth cloud of label_view, a second slot that stays across upload_cloud and
        every other call; an empty xyz clears it."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        assert xyz.shape == normals.shape
        self._check(lib().gpd_hip_upload_ground_truth(self._h, _ptr(xyz) if len(xyz) else None, _ptr(normals) if len(xyz) else None,
                                                      len(xyz)))

    def label_view(self, sample_rounds, min_positives, max_grasps_per_view, want_all_labels=False, capacity=None):
        """gpd_hip_label_view: one view of DataGenerator::generateData on the uploaded cloud against the uploaded ground truth.
        sample_rounds: i32 [max_rounds, samples_per_round], the sample indices of every round that may run.
        -> dict: images u8 [n,60,60,C], labels u8 [n], hands [n], src_index i32 [n] (positives first), rounds_run, num_candidates,
        num_positives, num_out, num_positives_out, gt_neighbourhoods, d2h_bytes, stage_ms [4], round_counts i32 [max_rounds, 2],
        and all_labels u8 [num_candidates] when asked for."""
        sr = np.ascontiguousarray(sample_rounds, np.int32)
        sr = sr.reshape(sr.shape[0] if sr.ndim > 1 else (1 if sr.size else 0), -1)
        rounds, per = sr.shape
        cap = 2 * (max(int(max_grasps_per_view), 0) // 2) if capacity is None else int(capacity)
        Cn = self.params.image_num_channels
        img = np.zeros((max(cap, 1), 60, 60, Cn), np.uint8)
        lab = np.zeros(max(cap, 1), np.uint8)
        hands = np.zeros(max(cap, 1), HAND_DTYPE)
        src = np.zeros(max(cap, 1), np.int32)
        counts = np.zeros((max(rounds, 1), 2), np.int32)
        all_cap = rounds * per * self.n_slots if want_all_labels else 0
        all_lab = np.zeros(max(all_cap, 1), np.uint8) if want_all_labels else None
        j = LabelViewJob()
        j.sample_indices, j.samples_per_round, j.max_rounds = _ptr(sr), per, rounds
        j.min_positives, j.max_grasps_per_view = int(min_positives), int(max_grasps_per_view)
        j.images, j.labels, j.hands, j.src_index, j.capacity = _ptr(img), _ptr(lab), _ptr(hands), _ptr(src), cap
        j.all_labels, j.all_labels_capacity, j.round_counts = _ptr(all_lab), all_cap, _ptr(counts)
        self._check(lib().gpd_hip_label_view(self._h, C.byref(j)))
        n = j.num_out
        out = dict(images=img[:n].copy(), labels=lab[:n].copy(), hands=hands[:n].copy(), src_index=src[:n].copy(),
                   rounds_run=int(j.rounds_run), num_candidates=int(j.num_candidates), num_positives=int(j.num_positives),
                   num_out=int(n), num_positives_out=int(j.num_positives_out), gt_neighbourhoods=int(j.gt_neighbourhoods),
                   d2h_bytes=int(j.d2h_bytes), stage_ms=[float(x) for x in j.stage_ms], round_counts=counts[:rounds].copy())
        if want_all_labels:
            out["all_labels"] = all_lab[: j.num_candidates].copy()
        return out

    def detect_sis(self, sample_indices, num_iterations, num_samples, prob_rand_samples=0.3, sigma=0.02, sampling_method=0, min_score=0.0,
                   workspace=(-1, 1, -1, 1, -1, 1), min_inliers=0, remove_inliers=False, seed=0, proposal_block=0, capacity=None):
        """gpd_hip_detect_sis: SequentialImportanceSampling::detectGrasps on the uploaded cloud, the rounds kept on the device.
        sample_indices: the initial pass (also the source of the uniform proposals).
        -> dict: hands [n] (score > min_score, clustered when min_inliers > 0), samples f64 [rounds_run, num_samples, 3], centres f64
        [num_sets, 3], round_counts i32 [1 + num_iterations, 4] (live sets, candidates, Gaussian / uniform proposals consumed),
        rounds_run, num_sets, num_candidates, num_hands, stage_ms [4] (draw, search, images + accumulate, LeNet + select +
        cluster), d2h_bytes."""
        si = np.ascontiguousarray(sample_indices, np.int32).reshape(-1)
        its, per = int(num_iterations), int(num_samples)
        total = len(si) + max(its, 0) * max(per, 0)
        cap = total * self.n_slots if capacity is None else int(capacity)
        hands = np.zeros(max(cap, 1), HAND_DTYPE)
        samples = np.zeros((max(its, 1), max(per, 1), 3), np.float64)
        centres = np.zeros((max(total, 1), 3), np.float64)
        counts = np.zeros((1 + max(its, 0), 4), np.int32)
        j = SisJob()
        j.sample_indices, j.num_init_samples = _ptr(si) if len(si) else None, len(si)
        j.num_iterations, j.num_samples, j.sampling_method = its, per, int(sampling_method)
        j.prob_rand_samples, j.sigma, j.min_score = float(prob_rand_samples), float(sigma), float(min_score)
        j.workspace = (C.c_double * 6)(*[float(v) for v in workspace])
        j.min_inliers, j.remove_inliers = int(min_inliers), int(bool(remove_inliers))
        j.seed, j.proposal_block = int(seed) & 0xFFFFFFFF, int(proposal_block)
        j.hands, j.capacity = (_ptr(hands) if cap > 0 else None), cap
        j.samples_out, j.centres_out, j.centres_capacity, j.round_counts = _ptr(samples), _ptr(centres), total, _ptr(counts)
        rc = lib().gpd_hip_detect_sis(self._h, C.byref(j))
        self.last_sis_num_hands = int(j.num_hands)
        self._check(rc)
        r = int(j.rounds_run)
        return dict(hands=hands[: j.num_hands].copy(), samples=samples[:r, :per].copy() if its > 0 else np.zeros((0, per, 3)),
                    centres=centres[: j.num_sets].copy(), round_counts=counts.copy(), rounds_run=r, num_sets=int(j.num_sets),
                    num_candidates=int(j.num_candidates), num_hands=int(j.num_hands), stage_ms=[float(x) for x in j.stage_ms],
                    d2h_bytes=int(j.d2h_bytes))

    def search(self, sample_indices):
        """generateGraspCandidateSets -> hands[n_sets, n_slots]."""
        si = np.ascontiguousarray(sample_indices, np.int32)
        hands = np.empty((len(si), self.n_slots), HAND_DTYPE)  # rows [0, num_sets) are written by the call
        ns = C.c_int(0)
        self._check(lib().gpd_hip_search(self._h, _ptr(si), len(si), _ptr(hands), C.byref(ns)))
        return hands[: ns.value].copy()

    def search_samples(self, samples_xyz):
        """generateGraspCandidateSets for samples given by coordinates (f64 [S,3])."""
        sm = np.ascontiguousarray(samples_xyz, np.float64).reshape(-1, 3)
        hands = np.empty((len(sm), self.n_slots), HAND_DTYPE)
        ns = C.c_int(0)
        self._check(lib().gpd_hip_search_samples(self._h, _ptr(sm), len(sm), _ptr(hands), C.byref(ns)))
        return hands[: ns.value].copy()

    def detect_samples(self, samples_xyz):
        sm = np.ascontiguousarray(samples_xyz, np.float64).reshape(-1, 3)
        hands = np.empty((len(sm), self.n_slots), HAND_DTYPE)
        ns, nc = C.c_int(0), C.c_int(0)
        self._check(lib().gpd_hip_detect_samples(self._h, _ptr(sm), len(sm), _ptr(hands), C.byref(ns), C.byref(nc)))
        return hands[: ns.value].copy(), nc.value

    def reevaluate(self, hands):
        """HandSearch::reevaluateHypotheses on the uploaded cloud -> (labels int32 [n], rewritten hands [n])."""
        h = np.ascontiguousarray(hands, HAND_DTYPE).reshape(-1).copy()
        labels = np.zeros(len(h), np.int32)
        self._check(lib().gpd_hip_reevaluate(self._h, _ptr(h), len(h), _ptr(labels)))
        return labels, h

    def images(self, hands, download=True):
        """ImageGenerator::createImages -> (images[n,60,60,C] or None, cand_index[n])."""
        hands = np.ascontiguousarray(hands)
        nv = int(hands["valid"].astype(bool).sum())
        Cn = self.params.image_num_channels
        img = np.zeros((nv, 60, 60, Cn), np.uint8) if download else None
        cand = np.zeros(max(nv, 1), np.int32)
        n = C.c_int(0)
        self._check(lib().gpd_hip_images(self._h, _ptr(hands), hands.shape[0], _ptr(img), _ptr(cand), C.byref(n)))
        assert n.value == nv
        return img, cand[:nv]

    def _given(self, hands):
        hands = np.ascontiguousarray(hands, HAND_DTYPE)
        if hands.ndim != 2 or hands.shape[1] != self.n_slots:
            raise ValueError("hands must be [num_sets, %d] records, set-major" % self.n_slots)
        return hands, int(hands["valid"].astype(bool).sum())

    def images_given(self, hands, lcg_base=0, download=True):
        """gpd_hip_images_given: ImageGenerator::createImages for hand sets the caller supplies (given_check is the domain), on the
        uploaded cloud -> (images [n,60,60,C] or None: kept on the device for score(None, n), cand_index [n], lcg_draws)."""
        hands, nv = self._given(hands)
        img = np.zeros((nv, 60, 60, self.params.image_num_channels), np.uint8) if download else None
        cand = np.zeros(max(nv, 1), np.int32)
        n, draws = C.c_int(0), C.c_uint64(0)
        self._check(lib().gpd_hip_images_given(self._h, _ptr(hands), hands.shape[0], int(lcg_base), _ptr(img), _ptr(cand), C.byref(n),
                                               C.byref(draws)))
        assert n.value == nv
        return img, cand[:nv], int(draws.value)

    def score_given(self, hands, lcg_base=0):
        """gpd_hip_score_given: images_given + the LeNet in the context's mode -> (a copy of hands with `score` written into the
        valid records, scores f32 [n], cand_index [n], lcg_draws)."""
        hands, nv = self._given(hands)
        hands = hands.copy()
        scores = np.zeros(max(nv, 1), np.float32)
        cand = np.zeros(max(nv, 1), np.int32)
        n, draws = C.c_int(0), C.c_uint64(0)
        self._check(lib().gpd_hip_score_given(self._h, _ptr(hands), hands.shape[0], int(lcg_base), _ptr(scores), _ptr(cand), C.byref(n),
                                              C.byref(draws)))
        assert n.value == nv
        return hands, scores[:nv], cand[:nv], int(draws.value)

    def detect(self, sample_indices):
        """detectGrasps steps 1-4 -> (hands[n_sets, n_slots] with scores, n_candidates)."""
        si = np.ascontiguousarray(sample_indices, np.int32)
        hands = np.empty((len(si), self.n_slots), HAND_DTYPE)  # rows [0, num_sets) are written by the call
        ns, nc = C.c_int(0), C.c_int(0)
        self._check(lib().gpd_hip_detect(self._h, _ptr(si), len(si), _ptr(hands), C.byref(ns), C.byref(nc)))
        return hands[: ns.value], nc.value

    def detect_select(self, sample_indices, num_selected=0):
        """detectGrasps steps 1-4 (+ selectGrasps when num_selected > 0) -> (hands[k], n_sets, n_candidates):
        only the scored candidates (or the num_selected best, score descending) come back."""
        si = np.ascontiguousarray(sample_indices, np.int32)
        cap = len(si) * self.n_slots if num_selected == 0 else min(num_selected, len(si) * self.n_slots)
        hands = np.empty(max(cap, 1), HAND_DTYPE)
        ns, nc, nh = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(lib().gpd_hip_detect_select(self._h, _ptr(si), len(si), int(num_selected), _ptr(hands), cap,
                                                C.byref(ns), C.byref(nc), C.byref(nh)))
        return hands[: nh.value], ns.value, nc.value

    def _jobs(self, clouds, samples, num_selected):
        jobs = (DetectJob * len(clouds))()
        keep = []
        for j, cl, si in zip(jobs, clouds, samples):
            xyz = np.ascontiguousarray(cl["xyz"], np.float32)
            nrm = np.ascontiguousarray(cl["normals"], np.float32)
            P = len(xyz)
            cam = np.ascontiguousarray(cl["cam_source"], np.int32).reshape(-1, P)
            vp = np.ascontiguousarray(cl["view_points"], np.float64).reshape(-1, 3)
            si = np.ascontiguousarray(si, np.int32)
            cap = len(si) * self.n_slots if num_selected == 0 else min(num_selected, len(si) * self.n_slots)
            hands = np.empty(max(cap, 1), HAND_DTYPE)
            keep.append((xyz, nrm, cam, vp, si, hands))
            j.xyz, j.normals, j.cam_source, j.view_points = _ptr(xyz), _ptr(nrm), _ptr(cam), _ptr(vp)
            j.sample_indices, j.hands = _ptr(si), _ptr(hands)
            j.num_points, j.num_cams, j.num_samples = P, cam.shape[0], len(si)
            j.num_selected, j.hands_capacity = int(num_selected), cap
        return jobs, keep

    def raw_batch(self, scans, samples_xyz, workspace=None, voxel_size=0.003, normals_radius=0.03, num_selected=0,
                  refine_normals_k=0, sample_above_plane=False, num_draws=0, sample_seed=0, outlier_mean_k=0, outlier_stddev_mult=1.0):
        """The job array of gpd_hip_detect_batch for RAW scans (dicts with xyz, cam_source, view_points): preprocessPointCloud
        (workspace cut, voxeliser, normals, refineNormals when refine_normals_k > 0) on the device, search at the given sample
        coordinates (one f64 [S, 3] array per scan).  samples_xyz[i] is None: the index route — sampleAbovePlane when asked for,
        then Cloud::subsample(num_draws) on the stream seeded with sample_seed; the sample indices searched arrive in keep[i][7].
        outlier_mean_k > 0: removeStatisticalOutliers(outlier_mean_k, outlier_stddev_mult) after the voxeliser, before the normals.
        refine_normals_k, sample_above_plane, num_draws, sample_seed, outlier_mean_k and outlier_stddev_mult take one value for all
        scans or a sequence with one per scan."""
        jobs = (DetectJob * len(scans))()
        keep = []
        ws = None if workspace is None else np.ascontiguousarray(workspace, np.float64)

        def per_scan(v, i):
            return v[i] if isinstance(v, (list, tuple, np.ndarray)) else v

        for i, (j, cl, sm) in enumerate(zip(jobs, scans, samples_xyz)):
            xyz = np.ascontiguousarray(cl["xyz"], np.float32)
            P = len(xyz)
            cam = np.ascontiguousarray(cl["cam_source"], np.int32).reshape(-1, P)
            vp = np.ascontiguousarray(cl["view_points"], np.float64).reshape(-1, 3)
            draws = int(per_scan(num_draws, i))
            if sm is None:
                S, drawn = max(draws, 0), np.zeros(max(draws, 1), np.int32)
            else:
                sm = np.ascontiguousarray(sm, np.float64).reshape(-1, 3)
                S, drawn = len(sm), None
            cap = S * self.n_slots if num_selected == 0 else min(num_selected, S * self.n_slots)
            hands = np.empty(max(cap, 1), HAND_DTYPE)
            keep.append((xyz, None, cam, vp, sm, hands, ws, drawn))
            j.xyz, j.cam_source, j.view_points, j.hands = _ptr(xyz), _ptr(cam), _ptr(vp), _ptr(hands)
            j.sample_xyz, j.workspace = _ptr(sm), _ptr(ws)
            j.num_points, j.num_cams, j.num_samples = P, cam.shape[0], 0 if sm is None else len(sm)
            j.num_selected, j.hands_capacity = int(num_selected), cap
            j.raw, j.voxel_size, j.normals_radius = 1, float(voxel_size), float(normals_radius)
            j.refine_normals_k, j.sample_above_plane = int(per_scan(refine_normals_k, i)), int(bool(per_scan(sample_above_plane, i)))
            j.num_draws, j.sample_seed = draws, int(per_scan(sample_seed, i)) & 0xFFFFFFFF
            j.samples_out = _ptr(drawn)
            j.outlier_mean_k, j.outlier_stddev_mult = int(per_scan(outlier_mean_k, i)), float(per_scan(outlier_stddev_mult, i))
        return jobs, keep

    def batch(self, clouds, samples, num_selected=0):
        """The job array of gpd_hip_detect_batch with its input views and output buffers, built once and reusable: a
        caller that runs batch after batch (bench.py's passes) allocates nothing per call."""
        return self._jobs(clouds, samples, num_selected)

    def run_batch(self, batch):
        """gpd_hip_detect_batch on a prepared batch -> list of (hands[k], n_sets, n_candidates, stage_ms[3]) in cloud
        order; the hands are views into the batch's own buffers (overwritten by the next run)."""
        jobs, keep = batch
        self._check(lib().gpd_hip_detect_batch(self._h, jobs, len(jobs)))
        # where the host was per cloud (ms since entry) and the buffer growths booked on it: kept for the caller that asks
        self.last_batch_timeline = [([float(x) for x in j.host_ms], int(j.allocs)) for j in jobs]
        return [(k[5][: j.num_hands], j.num_sets, j.num_candidates, [float(x) for x in j.stage_ms])
                for j, k in zip(jobs, keep)]

    def detect_batch(self, clouds, samples, num_selected=0):
        """detect_grasps over independent clouds (two in flight per context).  clouds: dicts with xyz, normals,
        cam_source, view_points; samples: one int32 index array per cloud.
        -> list of (hands[k], n_sets, n_candidates, stage_ms[3]) in cloud order."""
        return self.run_batch(self.batch(clouds, samples, num_selected))

    def reserve(self, max_points, max_cams=1, max_samples=0, max_candidates=0, max_selected=0):
        """gpd_hip_reserve: size every buffer of the context once (no allocation in later calls within these sizes)."""
        self._check(lib().gpd_hip_reserve(self._h, int(max_points), int(max_cams), int(max_samples), int(max_candidates), int(max_selected)))

    def detect_batch_multi(self, others, clouds, samples, num_selected=0):
        """gpd_hip_detect_batch_multi over this context and `others` (one host thread per context, cloud i ->
        context i mod G).  Same return value as detect_batch."""
        ctxs = [self] + list(others)
        jobs, keep = self._jobs(clouds, samples, num_selected)
        arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
        self._check(lib().gpd_hip_detect_batch_multi(arr, len(ctxs), jobs, len(clouds)))
        return [(k[5][: j.num_hands], j.num_sets, j.num_candidates, [float(x) for x in j.stage_ms])
                for j, k in zip(jobs, keep)]

    def detect_sharded(self, others, cloud, samples, split=None):
        """gpd_hip_detect_sharded: ONE cloud, its samples cut into len(others) + 1 contiguous ranges (at the indices `split`, default
        equal shares), range g on context g.  -> (hands of all ranges concatenated, per-shard (n_sets, n_candidates, lcg_base,
        lcg_draws))."""
        ctxs = [self] + list(others)
        G = len(ctxs)
        si = np.ascontiguousarray(samples, np.int32)
        cuts = [0] + (list(split) if split is not None else [len(si) * g // G for g in range(1, G)]) + [len(si)]
        parts = [si[cuts[g]:cuts[g + 1]] for g in range(G)]
        jobs, keep = self._jobs([cloud] * G, parts, 0)
        arr = (C.c_void_p * G)(*[c._h for c in ctxs])
        self._check(lib().gpd_hip_detect_sharded(arr, G, jobs))
        hands = np.concatenate([k[5][: j.num_hands] for j, k in zip(jobs, keep)])
        return hands, [(j.num_sets, j.num_candidates, int(j.lcg_base), int(j.lcg_draws)) for j in jobs]

    def stage_ms(self):
        ms = np.zeros(3, np.float32)
        self._check(lib().gpd_hip_last_stage_ms(self._h, _ptr(ms)))
        return ms

    def replay(self, stages=3):
        """Re-run images (1) and/or LeNet (2) on the device-resident candidate list (async)."""
        self._check(lib().gpd_hip_replay(self._h, int(stages)))

    def replay_times(self, n_scores=0):
        """Synchronise -> (image_ms_sum, lenet_ms_sum, launches, scores or None)."""
        ms = np.zeros(2, np.float32)
        n = C.c_int(0)
        sc = np.zeros(n_scores, np.float32) if n_scores else None
        self._check(lib().gpd_hip_replay_times(self._h, _ptr(ms), C.byref(n), _ptr(sc)))
        return float(ms[0]), float(ms[1]), n.value, sc

    def replay_kernel_ms(self):
        """Summed HIP-event time of conv1, conv2, ip1, ip2 over the replays of the last replay_times()."""
        ms = np.zeros(4, np.float32)
        self._check(lib().gpd_hip_replay_kernel_ms(self._h, _ptr(ms)))
        return [float(x) for x in ms]

    def conv1_stats(self, reset=True):
        """(executed, looked-at) (chunk, channel) pairs of conv1's launches since the last reset."""
        out = np.zeros(2, np.uint64)
        self._check(lib().gpd_hip_conv1_stats(self._h, _ptr(out), int(bool(reset))))
        return int(out[0]), int(out[1])

    def images_stats(self):
        out = np.zeros(4, np.int64)
        self._check(lib().gpd_hip_last_images_stats(self._h, _ptr(out)))
        return dict(candidates=int(out[0]), sets=int(out[1]), sum_set_ni=int(out[2]), sum_cand_ni=int(out[3]))

    def fallbacks(self):
        """Slow paths of the last search / image stage: list capacity, candidates redone by the large shadow / points
        kernels, LeNet passes."""
        out = np.zeros(4, np.int64)
        self._check(lib().gpd_hip_last_fallbacks(self._h, _ptr(out)))
        return dict(neighbourhood_list_capacity=int(out[0]), large_shadow_kernel_candidates=int(out[1]),
                    large_points_kernel_candidates=int(out[2]), lenet_passes=int(out[3]))

    def image_routes(self):
        """Which image kernels the last image launch sent each candidate through (tests only) -> (route int32 [n], info):
        route bit 1 = queued for the large shadow instantiation, 2 = queued again for the general shadow kernel, 4 = queued
        for the large points kernel; info: candidates, window_class (0 default, 1 wide, 2 huge), set_mode
        (shadow_set_kernel's, -1: none), status (capacity flags), and the caps pt_cap, pt_cap_big, sh_cap, sh_cap_big."""
        n = self.images_stats()["candidates"]
        route = np.zeros(max(n, 1), np.int32)
        info = np.zeros(8, np.int64)
        self._check(lib().gpd_hip_last_image_routes(self._h, _ptr(route), len(route), _ptr(info)))
        keys = ("candidates", "window_class", "set_mode", "status", "pt_cap", "pt_cap_big", "sh_cap", "sh_cap_big")
        info = {k: int(v) for k, v in zip(keys, info)}
        return route[: info["candidates"]].copy(), info

    def normals_routes(self):
        """Which route every point took through the last estimate_normals (tests only) -> (count int32 [P], info): count =
        neighbours found per point by original index, self included; info: points, tiles, queued (more than 1024 neighbours),
        queued_lds / queued_arena (where their keys were sorted), attempts (2: the arena grew and the run was repeated),
        arena_slots (its capacity after the call, 8-byte slots), centroid_chains (points not queued whose centroid chains were walked)."""
        count = np.zeros(max(getattr(self, "_num_points", 0), 1), np.int32)  # (no upload yet: the call refuses)
        info = np.zeros(8, np.int64)
        self._check(lib().gpd_hip_last_normals_routes(self._h, _ptr(count), len(count), _ptr(info)))
        keys = ("points", "tiles", "queued", "queued_lds", "queued_arena", "attempts", "arena_slots", "centroid_chains")
        info = {k: int(v) for k, v in zip(keys, info)}
        return count[: info["points"]].copy(), info

    def centre_chains(self):
        """(sample, coordinate) pairs of the last search whose neighbourhood centre took the serial fp64 chain (the order-free sum
        inside the neighbourhood kernel could not be certified exact)."""
        out = C.c_longlong(0)
        self._check(lib().gpd_hip_last_centre_chains(self._h, C.byref(out)))
        return int(out.value)

    def find_clusters(self, hands, scores, min_inliers=1, remove_inliers=False):
        """Clustering::findClusters on the device -> (cluster records, scores f64, seed index)."""
        hands = np.ascontiguousarray(hands, HAND_DTYPE).reshape(-1)
        scores = np.ascontiguousarray(scores, np.float64)
        assert len(scores) == len(hands)
        n = len(hands)
        out = np.zeros(max(n, 1), HAND_DTYPE)
        osc = np.zeros(max(n, 1), np.float64)
        src = np.zeros(max(n, 1), np.int32)
        k = C.c_int(0)
        self._check(lib().gpd_hip_find_clusters(self._h, _ptr(hands), _ptr(scores), n, int(min_inliers), int(bool(remove_inliers)), _ptr(out),
                                                _ptr(osc), _ptr(src), C.byref(k)))
        return out[: k.value].copy(), osc[: k.value].copy(), src[: k.value].copy()

    def preprocess_cloud(self, xyz, cam_source=None, workspace=None, voxel_size=0.003):
        """Cloud::filterWorkspace (points) + Cloud::voxelizeCloud on the device ->
        (xyz f32 [M,3], cam_source i32 [cams,M], input index per output point i32 [M], kernel ms)."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        P = len(xyz)
        cam = np.zeros((0, P), np.int32) if cam_source is None else np.ascontiguousarray(cam_source, np.int32).reshape(-1, P)
        ws = None if workspace is None else np.ascontiguousarray(workspace, np.float64)
        assert ws is None or ws.shape == (6,)
        out = np.zeros((P, 3), np.float32)
        cam_out = np.zeros((cam.shape[0], P), np.int32).reshape(-1)
        src = np.zeros(P, np.int32)
        n, ms = C.c_int(0), C.c_float(0)
        self._check(lib().gpd_hip_preprocess_cloud(self._h, _ptr(xyz) if P else None, _ptr(cam) if cam.size else None, P, cam.shape[0],
                                                   _ptr(ws) if ws is not None else None, float(voxel_size), _ptr(out) if P else None,
                                                   _ptr(cam_out) if cam.size else None, _ptr(src) if P else None, C.byref(n), C.byref(ms)))
        M = n.value
        return out[:M].copy(), cam_out[: cam.shape[0] * M].reshape(cam.shape[0], M).copy(), src[:M].copy(), ms.value

    def estimate_normals(self, radius=0.03):
        """Cloud::calculateNormals on the uploaded cloud -> f32 [P,3] (also kept on the device)."""
        P = self._num_points
        out = np.zeros((P, 3), np.float32)
        self._check(lib().gpd_hip_estimate_normals(self._h, float(radius), _ptr(out)))
        return out

    def sample_above_plane(self, threshold=0.01, max_iterations=50, probability=0.99, optimize=True):
        """Cloud::sampleAbovePlane on the uploaded cloud (RANSAC support plane) ->
        (indices off the plane i32 ascending — empty: the fit failed —, plane coefficients f32 [4], inliers, iterations)."""
        P = self._num_points
        idx = np.zeros(max(P, 1), np.int32)
        coeffs = np.zeros(4, np.float32)
        n, inl, its = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(lib().gpd_hip_sample_above_plane(self._h, float(threshold), int(max_iterations), float(probability), int(bool(optimize)),
                                                     _ptr(idx), C.byref(n), _ptr(coeffs), C.byref(inl), C.byref(its)))
        return idx[: n.value].copy(), coeffs, int(inl.value), int(its.value)

    def refine_normals(self, k, max_iterations=15, convergence_threshold=1e-5):
        """Cloud::refineNormals(k) on the normals of the uploaded (or last estimated) cloud (kNN + NormalRefinement);
        the result replaces the device copy, so a detect that follows uses it -> (normals f32 [P,3] (NaN: a singularity),
        passes run, the stop rule's mean dot product of every pass f32 [passes], normals with a non-finite component).
        self.last_refine_ms: kNN kernel, refinement passes launched, the whole call (ms)."""
        P = self._num_points
        out = np.zeros((P, 3), np.float32)
        ddots = np.zeros(max(int(max_iterations), 1), np.float32)
        ms = np.zeros(3, np.float32)
        its, nan = C.c_int(0), C.c_int(0)
        self._check(lib().gpd_hip_refine_normals(self._h, int(k), int(max_iterations), float(convergence_threshold), _ptr(out), C.byref(its),
                                                 _ptr(ddots), C.byref(nan), _ptr(ms)))
        self.last_refine_ms = tuple(float(v) for v in ms)
        return out, int(its.value), ddots[: its.value].copy(), int(nan.value)

    def remove_statistical_outliers(self, mean_k=50, stddev_mult=1.0):
        """Cloud::removeStatisticalOutliers on the uploaded cloud (pcl::StatisticalOutlierRemoval): the kept points
        replace the cloud on the device, their normals and camera rows with them, so an estimate_normals / detect that follows
        runs on the kept cloud -> (kept input indices i32 ascending, stats f64 [3]: mean, stddev, threshold, mean neighbour
        distance of every input point f32 [N]).  self.last_outlier_ms: distance kernel, compaction, the whole call (ms)."""
        P = getattr(self, "_num_points", 0)  # (no upload yet: the call refuses)
        kept = np.zeros(max(P, 1), np.int32)
        stats = np.zeros(3, np.float64)
        dist = np.zeros(max(P, 1), np.float32)
        ms = np.zeros(3, np.float32)
        n = C.c_int(0)
        self._check(lib().gpd_hip_remove_statistical_outliers(self._h, int(mean_k), float(stddev_mult), _ptr(kept), C.byref(n), _ptr(stats),
                                                              _ptr(dist), _ptr(ms)))
        self.last_outlier_ms = tuple(float(v) for v in ms)
        self._num_points = int(n.value)
        return kept[: n.value].copy(), stats, dist[:P].copy()


def torch_state_shapes(channels):
    """The shapes of Net's eight tensors, in TORCH_KEYS order."""
    return ((20, int(channels), 5, 5), (20,), (50, 20, 5, 5), (50,), (500, 7200), (500,), (2, 500), (2,))


def _state_buffers(channels):
    arrs = [np.zeros(s, np.float32) for s in torch_state_shapes(channels)]
    return arrs, (C.c_void_p * 8)(*[a.ctypes.data for a in arrs])


def _state_pointers(state, channels):
    t = torch_state_arrays(state)
    arrs = [t[k] for k in TORCH_KEYS]
    for k, a, s in zip(TORCH_KEYS, arrs, torch_state_shapes(channels)):
        if a.size != int(np.prod(s)):
            raise ValueError("%s has %d elements, %d expected for %d channels" % (k, a.size, int(np.prod(s)), channels))
    return arrs, (C.c_void_p * 8)(*[a.ctypes.data for a in arrs])


def net_shape(channels, shape):
    """(F1, F2, H1) or (F1, F2, H1, H2) or a LenetShape -> the LenetShape at `channels` channels"""
    if isinstance(shape, LenetShape):
        if shape.channels != int(channels):
            raise ValueError("the shape has %d channels, %d expected" % (shape.channels, int(channels)))
        return shape
    w = [int(x) for x in shape]
    if len(w) not in (3, 4):
        raise ValueError("a network shape is (F1, F2, H1) or (F1, F2, H1, H2), not %r" % (shape,))
    return LenetShape(int(channels), w[0], w[1], w[2], w[3] if len(w) == 4 else 0)


def net_keys(shape):
    """The keys of the state of a network of `shape`: TORCH_KEYS, or TORCH_NET_KEYS with a third dense layer."""
    return TORCH_NET_KEYS if shape.fc2_out > 0 else TORCH_KEYS


def net_state_shapes(shape):
    """The shapes of the 8 or 10 tensors of a network of `shape` (a LenetShape), in net_keys order."""
    Cn, F1, F2, H1, H2 = shape.as_tuple()
    out = [(F1, Cn, 5, 5), (F1,), (F2, F1, 5, 5), (F2,), (H1, F2 * 144), (H1,)]
    return tuple(out + ([(H2, H1), (H2,), (2, H2), (2,)] if H2 > 0 else [(2, H1), (2,)]))


def net_sizes(shape):
    """gpd_hip_train_net_sizes: the element counts of the ten tensors (the last two 0 without a third dense layer; host only)."""
    n = (C.c_size_t * 10)()
    _lib_check(lib().gpd_hip_train_net_sizes(C.byref(shape), n))
    return [int(x) for x in n]


def _net_buffers(shape):
    arrs = [np.zeros(s, np.float32) for s in net_state_shapes(shape)]
    return arrs, _pointer_table(arrs)


def _net_pointers(state, shape):
    plain = {(str(k)[len("module."):] if str(k).startswith("module.") else str(k)): v for k, v in state.items()}
    arrs = []
    for k, want in zip(net_keys(shape), net_state_shapes(shape)):
        if k not in plain:
            raise KeyError("state dict has no %r (keys: %s)" % (k, sorted(plain)))
        v = plain[k]
        if hasattr(v, "detach"):
            v = v.detach().cpu().numpy()
        a = np.ascontiguousarray(v, np.float32)
        if a.size != int(np.prod(want)):
            raise ValueError("%s has %d elements, %d expected for %r" % (k, a.size, int(np.prod(want)), shape))
        arrs.append(a)
    return arrs, _pointer_table(arrs)


def train_default_params(channels=15, max_batch=64):
    p = TrainParams()
    lib().gpd_hip_train_default_params(C.byref(p))
    p.channels, p.max_batch = int(channels), int(max_batch)
    return p


def init_state(channels, seed=0, shape=None):
    """gpd_hip_train_init_state: a seeded initial state of Net, every tensor U(-1/sqrt(fan_in), 1/sqrt(fan_in)) (host only)
    -> {key: f32 array in torch layout}.  shape (net_shape): gpd_hip_train_net_init_state for a network of those widths, 8 or
    10 tensors."""
    if shape is not None:
        shape = net_shape(channels, shape)
        arrs, ptrs = _net_buffers(shape)
        _lib_check(lib().gpd_hip_train_net_init_state(C.byref(shape), int(seed) & 0xFFFFFFFF, ptrs))
        return dict(zip(net_keys(shape), arrs))
    if int(channels) not in (1, 3, 12, 15):
        raise GpdHipError("libgpd_hip error -1: init_state: %d channels (1, 3, 12 or 15)" % int(channels))
    arrs, ptrs = _state_buffers(channels)
    rc = lib().gpd_hip_train_init_state(int(channels), int(seed) & 0xFFFFFFFF, ptrs)
    if rc != 0:
        raise GpdHipError("libgpd_hip error %d: %s" % (rc, lib().gpd_hip_last_error().decode()))
    return dict(zip(TORCH_KEYS, arrs))


def _lib_check(rc):
    if rc != 0:
        raise GpdHipError("libgpd_hip error %d: %s" % (rc, lib().gpd_hip_last_error().decode()))


def train_default_recipe(which=0, **kw):
    """gpd_hip_train_default_recipe: 0 — today's trainer (Net, Adam, fixed rate); 1 — the reference's Caffe files (the network
    without conv ReLUs, SGD with momentum 0.9, lr_policy inv with gamma 1e-4 and power 0.75; their base_lr CAFFE_BASE_LR goes
    into TrainParams.lr).  kw: fields to change; lr_mult / decay_mult take eight values or a {tensor name: value} dict."""
    r = TrainRecipe()
    _lib_check(lib().gpd_hip_train_default_recipe(C.byref(r), int(which)))
    for k, v in kw.items():
        if k not in dict(TrainRecipe._fields_):
            raise TypeError("gpd_train_recipe has no field %r" % k)
        if k in ("lr_mult", "decay_mult"):
            cur = list(getattr(r, k))
            if isinstance(v, dict):
                for name, x in v.items():
                    cur[TORCH_KEYS.index(name)] = float(x)
            else:
                cur = [float(x) for x in v]
                if len(cur) != 8:
                    raise ValueError("%s takes eight values" % k)
            v = (C.c_double * 8)(*cur)
        setattr(r, k, v)
    return r


def init_xavier(channels, seed=0, shape=None):
    """gpd_hip_train_init_xavier: Caffe's xavier filler from the project's seeded stream — weights U(-sqrt(3 / fan_in),
    sqrt(3 / fan_in)), biases 0 (host only) -> {key: f32 array in torch layout}.  shape: as in init_state."""
    if shape is not None:
        shape = net_shape(channels, shape)
        arrs, ptrs = _net_buffers(shape)
        _lib_check(lib().gpd_hip_train_net_init_xavier(C.byref(shape), int(seed) & 0xFFFFFFFF, ptrs))
        return dict(zip(net_keys(shape), arrs))
    if int(channels) not in (1, 3, 12, 15):
        raise GpdHipError("libgpd_hip error -1: init_xavier: %d channels (1, 3, 12 or 15)" % int(channels))
    arrs, ptrs = _state_buffers(channels)
    _lib_check(lib().gpd_hip_train_init_xavier(int(channels), int(seed) & 0xFFFFFFFF, ptrs))
    return dict(zip(TORCH_KEYS, arrs))


def learning_rate(recipe, base_lr, it):
    """gpd_hip_train_learning_rate: the rate of update `it` (0-based) under the recipe's policy, as the step uses it -> np.float32"""
    lr = C.c_float(0)
    _lib_check(lib().gpd_hip_train_learning_rate(C.byref(recipe), float(base_lr), int(it), C.byref(lr)))
    return np.float32(lr.value)


class Trainer:
    """One gpd_hip_trainer on a Context's device and stream.  Without a recipe: Net (pytorch/network.py) under softmax
    cross-entropy and Adam, as pytorch/train_net3.py trains it.  recipe (train_default_recipe): the network with or without conv
    ReLUs, Adam or Caffe's SGD, a learning-rate policy.  shape = (F1, F2, H1) or (F1, F2, H1, H2): a network of those widths
    (gpd_hip_train_create_net; H2 > 0: NetCCFFF, whose state has the ten TORCH_NET_KEYS) at the params' channel count; None: the
    stock widths through the stock entries.  The state travels as a dict of numpy arrays in torch layout, both ways.  Close it
    before its context."""

    def __init__(self, ctx, params=None, recipe=None, shape=None, **kw):
        self.params = params if params is not None else train_default_params(ctx.params.image_num_channels)
        self.recipe = recipe
        for k, v in kw.items():
            if k not in dict(TrainParams._fields_):
                raise TypeError("gpd_train_params has no field %r" % k)
            setattr(self.params, k, v)
        self.channels = int(self.params.channels)
        self._ctx = ctx  # keeps the context (the stream) alive
        self._h = C.c_void_p()
        self._net = shape is not None  # the entries with tables of 10
        self.shape = net_shape(self.channels, shape) if self._net else LenetShape(self.channels, 20, 50, 500, 0)
        self.keys = net_keys(self.shape)
        if self._net:
            self._check(lib().gpd_hip_train_create_net(ctx._h, C.byref(self.params), C.byref(recipe) if recipe is not None else None,
                                                       C.byref(self.shape), C.byref(self._h)))
        elif recipe is None:
            self._check(lib().gpd_hip_train_create(ctx._h, C.byref(self.params), C.byref(self._h)))
        else:
            self._check(lib().gpd_hip_train_create_recipe(ctx._h, C.byref(self.params), C.byref(recipe), C.byref(self._h)))
        self.caffe_network = recipe is not None and recipe.network == NET_CAFFE
        self.sgd = recipe is not None and recipe.solver == SOLVER_SGD

    _check = Context._check

    def close(self):
        if self._h:
            lib().gpd_hip_train_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _buffers(self):
        return _net_buffers(self.shape) if self._net else _state_buffers(self.channels)

    def _pointers(self, state):
        return _net_pointers(state, self.shape) if self._net else _state_pointers(state, self.channels)

    def _entry(self, name):
        """gpd_hip_train_<name>, or gpd_hip_train_net_<name> for a trainer made with a shape"""
        return getattr(lib(), ("gpd_hip_train_net_" if self._net else "gpd_hip_train_") + name)

    def set_state(self, state):
        """The tensors of self.keys; the solver's buffers (Adam's moments, SGD's history) and the update count start again."""
        arrs, ptrs = self._pointers(state)
        self._check(self._entry("set_state")(self._h, ptrs))

    def get_state(self):
        arrs, ptrs = self._buffers()
        self._check(self._entry("get_state")(self._h, ptrs))
        return dict(zip(self.keys, arrs))

    def get_solver_state(self):
        """-> dict(count = updates since set_state, m = {key: array}: Adam's exp_avg or SGD's history, v = Adam's exp_avg_sq or None)"""
        m, mp = self._buffers()
        v, vp = self._buffers() if not self.sgd else (None, None)
        n = C.c_longlong(0)
        self._check(self._entry("get_solver_state")(self._h, mp, vp, C.byref(n)))
        return dict(count=int(n.value), m=dict(zip(self.keys, m)), v=dict(zip(self.keys, v)) if v is not None else None)

    def set_solver_state(self, solver_state):
        """What get_solver_state returned, after set_state: the run continues byte for byte."""
        m, mp = self._pointers(solver_state["m"])
        v, vp = (None, None) if self.sgd or solver_state.get("v") is None else self._pointers(solver_state["v"])
        self._check(self._entry("set_solver_state")(self._h, mp, vp, int(solver_state["count"])))

    def set_data(self, images, labels, which=0):
        """The resident set `which` (0: training, 1: test): images u8 [n,60,60,C], labels u8 [n] of 0 / 1."""
        images = np.ascontiguousarray(images, np.uint8)
        labels = np.ascontiguousarray(labels, np.uint8).reshape(-1)
        if images.shape != (len(labels), 60, 60, self.channels):
            raise ValueError("images %s do not match %d labels of %d channels" % (images.shape, len(labels), self.channels))
        self._check(lib().gpd_hip_train_set_data(self._h, int(which), _ptr(images), _ptr(labels), len(labels)))

    def _images_labels(self, images, labels):
        images = np.ascontiguousarray(images, np.uint8)
        labels = np.ascontiguousarray(labels, np.uint8).reshape(-1)
        if images.shape != (len(labels), 60, 60, self.channels):
            raise ValueError("images %s do not match %d labels of %d channels" % (images.shape, len(labels), self.channels))
        return images, labels

    def reserve(self, capacity, which=0):
        """gpd_hip_train_reserve: room for max(capacity, n) images in set `which`; the images of the set stay."""
        self._check(lib().gpd_hip_train_reserve(self._h, int(which), int(capacity)))

    def count(self, which=0):
        """-> (images in set `which`, images its pool has room for)"""
        n, cap = C.c_int(0), C.c_int(0)
        self._check(lib().gpd_hip_train_count(self._h, int(which), C.byref(n), C.byref(cap)))
        return int(n.value), int(cap.value)

    def append_data(self, images, labels, which=0):
        """gpd_hip_train_append_data: host images u8 [n,60,60,C] and labels u8 [n] behind the last image of set `which` -> the
        position of the first appended image."""
        images, labels = self._images_labels(images, labels)
        first = self.count(which)[0]
        self._check(lib().gpd_hip_train_append_data(self._h, int(which), _ptr(images), _ptr(labels), len(labels)))
        return first

    def get_data(self, first=0, count=None, which=0):
        """gpd_hip_train_get_data: images [first, first + count) of set `which` (count None: to the end) -> (images u8
        [count,60,60,C], labels u8 [count])."""
        count = self.count(which)[0] - int(first) if count is None else int(count)
        images = np.zeros((max(count, 0), 60, 60, self.channels), np.uint8)
        labels = np.zeros(max(count, 0), np.uint8)
        self._check(lib().gpd_hip_train_get_data(self._h, int(which), int(first), count, _ptr(images), _ptr(labels)))
        return images, labels

    def reorder(self, first, order, which=0):
        """gpd_hip_train_reorder: images and labels of [first, first + len(order)) become new[k] = old[first + order[k]], on the
        device; `order` is a permutation of 0 .. len(order) - 1."""
        order = np.ascontiguousarray(order, np.int32).reshape(-1)
        self._check(lib().gpd_hip_train_reorder(self._h, int(which), int(first), len(order), _ptr(order)))

    def append_view(self, ctx, sample_rounds, min_positives, max_grasps_per_view, which=0, want_all_labels=False):
        """gpd_hip_train_append_view: Context.label_view on `ctx` (this trainer's context or another on the same device) whose kept
        images and labels go straight behind the last image of set `which` and never cross to the host -> label_view's dict
        without images, labels, hands and src_index, plus first: the position of the first appended image."""
        sr = np.ascontiguousarray(sample_rounds, np.int32)
        sr = sr.reshape(sr.shape[0] if sr.ndim > 1 else (1 if sr.size else 0), -1)
        rounds, per = sr.shape
        counts = np.zeros((max(rounds, 1), 2), np.int32)
        all_cap = rounds * per * ctx.n_slots if want_all_labels else 0
        all_lab = np.zeros(max(all_cap, 1), np.uint8) if want_all_labels else None
        j = LabelViewJob()
        j.sample_indices, j.samples_per_round, j.max_rounds = _ptr(sr), per, rounds
        j.min_positives, j.max_grasps_per_view = int(min_positives), int(max_grasps_per_view)
        j.all_labels, j.all_labels_capacity, j.round_counts = _ptr(all_lab), all_cap, _ptr(counts)
        first = self.count(which)[0]
        self._check(lib().gpd_hip_train_append_view(self._h, int(which), ctx._h, C.byref(j)))
        out = dict(first=first, rounds_run=int(j.rounds_run), num_candidates=int(j.num_candidates), num_positives=int(j.num_positives),
                   num_out=int(j.num_out), num_positives_out=int(j.num_positives_out), gt_neighbourhoods=int(j.gt_neighbourhoods),
                   d2h_bytes=int(j.d2h_bytes), stage_ms=[float(x) for x in j.stage_ms], round_counts=counts[:rounds].copy())
        if want_all_labels:
            out["all_labels"] = all_lab[: j.num_candidates].copy()
        return out

    def steps(self, indices, batch=None):
        """Steps of the recipe's solver (default Adam) on the training set: indices i32 [num_steps, batch] (or flat with `batch` given) -> each step's loss f32."""
        idx = np.ascontiguousarray(indices, np.int32)
        if batch is None:
            idx = idx.reshape(1, -1) if idx.ndim < 2 else idx
            batch = idx.shape[1]
        idx = idx.reshape(-1, int(batch))
        losses = np.zeros(len(idx), np.float32)
        self._check(lib().gpd_hip_train_steps(self._h, _ptr(idx), len(idx), int(batch), _ptr(losses)))
        return losses

    def gradients(self, indices):
        """Forward and backward of one batch, no update -> ({key: gradient}, loss)."""
        idx = np.ascontiguousarray(indices, np.int32).reshape(-1)
        arrs, ptrs = self._buffers()
        loss = C.c_float(0)
        self._check(self._entry("gradients")(self._h, _ptr(idx), len(idx), ptrs, C.byref(loss)))
        return dict(zip(self.keys, arrs)), float(loss.value)

    def apply(self, grads):
        """One step of the solver from the host's gradients (a dict like gradients() returns)."""
        arrs, ptrs = self._pointers(grads)
        self._check(self._entry("apply")(self._h, ptrs))

    def eval(self, indices=None, n=None, which=0):
        """Forward only over set `which`: the images `indices`, or the first n (default: all given by n) -> (logits f32 [n,2], num_correct)."""
        idx = None if indices is None else np.ascontiguousarray(indices, np.int32).reshape(-1)
        n = len(idx) if idx is not None else int(n)
        logits = np.zeros((max(n, 1), 2), np.float32)
        k = C.c_int(0)
        self._check(lib().gpd_hip_train_eval(self._h, int(which), _ptr(idx), n, _ptr(logits), C.byref(k)))
        return logits[:n], int(k.value)

    def step_timed(self, indices):
        """Measurement only: one step with an event behind every kernel -> [(kernel name, ms)]."""
        idx = np.ascontiguousarray(indices, np.int32).reshape(-1)
        ms = np.zeros(32, np.float32)
        k = C.c_int(0)
        self._check(lib().gpd_hip_train_step_timed(self._h, _ptr(idx), len(idx), _ptr(ms), len(ms), C.byref(k)))
        return [(lib().gpd_hip_train_kernel_name_of(self._h, i).decode(), float(ms[i])) for i in range(k.value)]

    def install(self, ctx=None, input_scale=None, net_mode=None):
        """get_state followed by Context.set_lenet_torch: the trained network becomes `ctx`'s (default: the trainer's own) scoring
        network, with the conv ReLUs on for Net and off for the Caffe network.  A network of other widths than the stock ones
        goes through Context.set_lenet_net onto the general route.  net_mode: Context.set_lenet_net_mode on `ctx` first (None
        leaves the context's mode alone; context state, so it is set whichever route the network takes)."""
        ctx = self._ctx if ctx is None else ctx
        if net_mode is not None:
            ctx.set_lenet_net_mode(net_mode)
        if self.shape.as_tuple()[1:] != (20, 50, 500, 0):
            ctx.set_lenet_net(self.get_state(), float(self.params.input_scale) if input_scale is None else input_scale,
                              conv_relu=not self.caffe_network)
            return
        ctx.set_lenet_torch(self.get_state(), float(self.params.input_scale) if input_scale is None else input_scale)
        if self.caffe_network:
            ctx.set_lenet_conv_relu(False)


# ---- training on several replicas (gpd_hip_train_group_*) ----

GROUP_OP_DTYPE = np.dtype([("kind", "<i4"), ("stream", "<i4"), ("peer", "<i4"), ("slice", "<i4"), ("event", "<i4")], align=False)
OP_BACKWARD, OP_WAIT, OP_RECORD, OP_COPY, OP_SUM, OP_UPDATE = range(6)


def train_group_mean(grads):
    """gpd_hip_train_group_mean: the mean of G equally shaped f32 arrays in rank order, ((g0 + g1) + ...) * f32(1 / G), every
    operation rounded to f32 (host only) -> f32 array of their shape."""
    arrs = [np.ascontiguousarray(g, np.float32) for g in grads]
    if not arrs or any(a.shape != arrs[0].shape for a in arrs):
        raise ValueError("train_group_mean takes at least one array, all of one shape")
    out = np.zeros(arrs[0].shape, np.float32)
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    _lib_check(lib().gpd_hip_train_group_mean(ptrs, len(arrs), arrs[0].size, _ptr(out)))
    return out


def train_group_slices(n, G):
    """gpd_hip_train_group_slices: the G + 1 boundaries of the slices of a buffer of n floats (host only) -> i64 [G + 1]."""
    first = np.zeros(max(int(G), 0) + 1, np.int64)
    _lib_check(lib().gpd_hip_train_group_slices(int(n), int(G), _ptr(first)))
    return first


def train_group_schedule(G, num_steps):
    """gpd_hip_train_group_schedule: the operations TrainerGroup.steps enqueues for num_steps steps of G replicas, in enqueue
    order (host only) -> GROUP_OP_DTYPE array."""
    k = C.c_int(0)
    _lib_check(lib().gpd_hip_train_group_schedule(int(G), int(num_steps), None, 0, C.byref(k)))
    ops = np.zeros(max(k.value, 1), GROUP_OP_DTYPE)
    _lib_check(lib().gpd_hip_train_group_schedule(int(G), int(num_steps), _ptr(ops), len(ops), C.byref(k)))
    return ops[: k.value].copy()


class TrainerGroup:
    """One gpd_hip_train_group over Trainers of one recipe and one set of hyper-parameters, each on a Context of its own (on
    different devices, or several on one).  A step runs every replica's batch and applies the mean of the gradients on every
    replica.  The group owns none of its trainers: close it before them."""

    def __init__(self, trainers):
        self.trainers = list(trainers)  # keeps them alive
        self._h = C.c_void_p()
        hs = (C.c_void_p * max(len(self.trainers), 1))(*[t._h.value for t in self.trainers])
        self._check(lib().gpd_hip_train_group_create(hs, len(self.trainers), C.byref(self._h)))

    _check = Context._check

    def __len__(self):
        return len(self.trainers)

    def close(self):
        if self._h:
            lib().gpd_hip_train_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def broadcast(self, src=0):
        """Replica src's parameters, solver buffers and update count into every other replica, device to device."""
        self._check(lib().gpd_hip_train_group_broadcast(self._h, int(src)))

    def steps(self, indices):
        """indices i32 [G, num_steps, batch], replica r's into its own resident training set -> (each step's loss f32
        [num_steps]: the mean of the replicas', each replica's losses f32 [G, num_steps])."""
        idx = np.ascontiguousarray(indices, np.int32)
        if idx.ndim != 3 or idx.shape[0] != len(self.trainers) or idx.shape[2] < 1:
            raise ValueError("indices %s are not [%d replicas, steps, batch]" % (idx.shape, len(self.trainers)))
        G, steps, batch = idx.shape
        ptrs = (C.c_void_p * G)(*[idx[r].ctypes.data for r in range(G)])
        losses, each = np.zeros(steps, np.float32), np.zeros((G, steps), np.float32)
        self._check(lib().gpd_hip_train_group_steps(self._h, ptrs, steps, batch, _ptr(losses), _ptr(each)))
        return losses, each

    def verify(self):
        """-> the 32-bit words of parameters and solver buffers that differ from replica 0's, plus the replicas whose update
        count differs: 0 for replicas in step."""
        n = C.c_longlong(0)
        self._check(lib().gpd_hip_train_group_verify(self._h, C.byref(n)))
        return int(n.value)

    def last_bytes(self):
        """-> (bytes moved between replicas, bytes moved between host and devices) by the last broadcast / steps / verify."""
        out = np.zeros(2, np.int64)
        self._check(lib().gpd_hip_train_group_last_bytes(self._h, _ptr(out)))
        return int(out[0]), int(out[1])
