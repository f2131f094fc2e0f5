"""The C-ABI library loads and exports every symbol include/gpd_hip.h declares (no GPU calls)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "gpd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gpd_hip_\w+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from gpd_amd import api
    L = api.lib()
    names = _declared()
    assert len(names) >= 12
    for n in names:
        assert hasattr(L, n), "libgpd_hip.so does not export " + n
    assert sorted(api.EXPORTS) == names


def test_default_params_match_reference_cfg():
    from gpd_amd import api
    p = api.default_params()
    # cfg/hand_geometry.cfg:8-12, cfg/image_geometry_15channels.cfg:8-12, cfg/eigen_params.cfg:34-42
    assert (p.finger_width, p.hand_outer_diameter, p.hand_depth, p.hand_height, p.init_bite) == (0.01, 0.12, 0.06, 0.02, 0.01)
    assert (p.volume_width, p.volume_depth, p.volume_height, p.image_size, p.image_num_channels) == (0.10, 0.06, 0.02, 60, 15)
    assert (p.num_orientations, p.num_finger_placements, p.num_hand_axes, p.hand_axes[0], p.deepen_hand) == (8, 10, 1, 2, 1)
    assert (p.friction_coeff, p.min_viable, p.max_aperture) == (20.0, 6, 0.085)


def test_no_gpu_means_error_not_fallback():
    """Without a GPU the product must fail loudly: no CPU path behind the C-ABI."""
    import torch
    if torch.cuda.is_available():
        return
    from gpd_amd import api
    try:
        api.Context(api.default_params())
    except api.GpdHipError as e:
        assert "libgpd_hip error" in str(e)
    else:
        raise AssertionError("Context() succeeded without a GPU")


def test_product_does_not_reference_the_oracle():
    bad = []
    for top in ("gpd_amd", "include"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".hip", ".cpp", ".h", "Makefile")):
                    txt = open(os.path.join(d, f)).read()
                    # neither the oracle, nor the reference build under oracle/_ref, nor the test-only third-party subsets
                    if re.search(r"import oracle|from oracle|libgpd_oracle|gpd_oracle_|libgpd_ref|gpd_ref_|oracle/shim|GPD_REF_SHIM", txt):
                        bad.append(f)
    assert not bad, bad


def test_release_library_reads_no_environment_and_links_no_profiler():
    """The shipped .so carries neither getenv switches nor the roctx dependency; the profiling
    build (libgpd_hip_prof.so, -DGPD_PROFILING) has both and exports the same C-ABI."""
    import subprocess
    rel = os.path.join(ROOT, "gpd_amd", "libgpd_hip.so")
    out = subprocess.run(["nm", "-D", "--undefined-only", rel], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in out and "roctx" not in out, out
    txt = "".join(open(os.path.join(ROOT, "gpd_amd", "csrc", f)).read() for f in os.listdir(os.path.join(ROOT, "gpd_amd", "csrc"))
                  if f.endswith((".hip", ".cpp")))
    assert not re.search(r"[^_\w]getenv\s*\(", txt), "a source of the release library calls getenv directly (use prof_env)"
    prof = os.path.join(ROOT, "gpd_amd", "libgpd_hip_prof.so")
    assert os.path.exists(prof)
    pout = subprocess.run(["nm", "-D", "--defined-only", prof], capture_output=True, text=True, check=True).stdout
    for n in _declared():
        assert n in pout


def test_shipped_sources_carry_no_experiment_switches():
    """The only conditional compilation in gpd_amd/csrc: the profiling build (GPD_PROFILING: roctx ranges, measurement switches read
    from the environment) and the host / device halves of the bf16 helpers that both sides of lenet_fast.hip use.  Timing experiments
    are built from patched copies (profiles/mkpatched.sh), not from switches in the product's sources."""
    allowed = {"GPD_PROFILING", "__HIP_DEVICE_COMPILE__"}
    d = os.path.join(ROOT, "gpd_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if not f.endswith((".hip", ".h", ".cpp")):
            continue
        for i, line in enumerate(open(os.path.join(d, f)), 1):
            m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b(.*)", line)
            if m:
                names = set(re.findall(r"[A-Za-z_][A-Za-z_0-9]*", m.group(2))) - {"defined"}
                assert names <= allowed, "%s:%d: %s" % (f, i, line.strip())


def test_image_routes_refuses_null_arguments():
    """gpd_hip_last_image_routes checks its arguments before it touches a context or the device: a null context, route
    buffer or info block, or a negative size, is GPD_ERR_INVALID (no GPU needed)."""
    from gpd_amd import api
    L = api.lib()
    route = (ctypes.c_int32 * 4)()
    info = (ctypes.c_longlong * 8)()
    not_a_context = ctypes.create_string_buffer(64)  # never dereferenced: the null buffer next to it is refused first
    assert L.gpd_hip_last_image_routes(None, route, 4, info) == -1
    assert L.gpd_hip_last_image_routes(not_a_context, None, 4, info) == -1
    assert L.gpd_hip_last_image_routes(not_a_context, route, 4, None) == -1
    assert L.gpd_hip_last_image_routes(not_a_context, route, -1, info) == -1
    assert b"bad argument" in L.gpd_hip_last_error()


def test_normals_routes_refuses_null_arguments():
    """gpd_hip_last_normals_routes, like its sibling, checks its arguments before it touches a context or the device: a null context,
    count buffer or info block, or a negative size, is GPD_ERR_INVALID (no GPU needed)."""
    from gpd_amd import api
    L = api.lib()
    count = (ctypes.c_int32 * 4)()
    info = (ctypes.c_longlong * 8)()
    not_a_context = ctypes.create_string_buffer(64)  # never dereferenced: the null buffer next to it is refused first
    assert L.gpd_hip_last_normals_routes(None, count, 4, info) == -1
    assert L.gpd_hip_last_error() == b"gpd_hip_last_normals_routes: bad argument"
    assert L.gpd_hip_last_normals_routes(not_a_context, None, 4, info) == -1
    assert L.gpd_hip_last_normals_routes(not_a_context, count, 4, None) == -1
    assert L.gpd_hip_last_normals_routes(not_a_context, count, -1, info) == -1
    assert L.gpd_hip_last_error() == b"gpd_hip_last_normals_routes: bad argument"
    assert list(count) == [0] * 4 and list(info) == [0] * 8  # nothing was written


def test_context_entries_refuse_null_arguments():
    """Every entry of context.hip, detect.hip, rounds.hip and given.hip that takes a context, and gpd_hip_detect_batch, refuses a
    null context, and a null in place of its first required pointer, with GPD_ERR_INVALID and the text "<entry>: bad argument" (gpd_hip_set_lenet_weights has
    said "null argument" from its first day), before it touches the context or the device (no GPU needed)."""
    from gpd_amd import api
    L = api.lib()
    ctx = ctypes.create_string_buffer(1 << 20)  # not a context, and never read: the null beside it is refused first
    buf = ctypes.create_string_buffer(4096)
    i = [ctypes.byref(ctypes.c_int()) for _ in range(4)]
    u64, f32 = ctypes.byref(ctypes.c_uint64()), ctypes.byref(ctypes.c_float())
    # entry -> the arguments behind the context, the first required pointer None
    cases = {
        "gpd_hip_reserve": None,
        "gpd_hip_set_lenet_weights": (15, None, buf, buf, buf, buf, buf, buf, buf),
        "gpd_hip_set_lenet_mode": None,
        "gpd_hip_set_lenet_conv_relu": None,
        "gpd_hip_lenet_debug": (0, 1, None),
        "gpd_hip_score": (buf, 1, None),
        "gpd_hip_upload_cloud": (None, buf, 1, buf, 1, buf),
        "gpd_hip_upload_ground_truth": (None, buf, 1),
        "gpd_hip_find_clusters": (buf, buf, 0, 0, 0, buf, buf, buf, None),
        "gpd_hip_preprocess_cloud": (buf, buf, 1, 1, buf, 0.01, buf, buf, buf, None, f32),
        "gpd_hip_estimate_normals": (0.01, None),
        "gpd_hip_sample_above_plane": (0.01, 10, 0.99, 0, None, i[0], buf, i[1], i[2]),
        "gpd_hip_refine_normals": (4, 1, 0.0, None, i[0], buf, i[1], buf),
        "gpd_hip_search": (None, 1, buf, i[0]),
        "gpd_hip_search_samples": (None, 1, buf, i[0]),
        "gpd_hip_reevaluate": (None, 1, buf),
        "gpd_hip_images": (None, 1, buf, buf, i[0]),
        "gpd_hip_detect": (None, 1, buf, i[0], i[1]),
        "gpd_hip_detect_samples": (None, 1, buf, i[0], i[1]),
        "gpd_hip_detect_select": (None, 1, 0, buf, 8, i[0], i[1], i[2]),
        "gpd_hip_label_view": (None,),
        "gpd_hip_detect_sis": (None,),
        "gpd_hip_images_given": (None, 1, 0, buf, buf, i[0], u64),
        "gpd_hip_score_given": (buf, 1, 0, buf, buf, None, u64),
        "gpd_hip_detect_batch": (None, 1),  # batch.hip: the one entry there that opens with the same helper
    }
    valid = {"gpd_hip_reserve": (1, 1, 0, 0, 0), "gpd_hip_set_lenet_mode": (0,), "gpd_hip_set_lenet_conv_relu": (0,),
             "gpd_hip_label_view": (ctypes.byref(api.LabelViewJob()),), "gpd_hip_detect_sis": (ctypes.byref(api.SisJob()),),
             "gpd_hip_detect_batch": (ctypes.byref(api.DetectJob()), 1)}
    for name, args in sorted(cases.items()):
        text = name.encode() + (b": null argument" if name == "gpd_hip_set_lenet_weights" else b": bad argument")
        fn = getattr(L, name)
        # a null context: the other arguments as good as they get without a device
        good = valid.get(name) or tuple(ctypes.cast(buf, ctypes.POINTER(ctypes.c_int)) if a is None else a for a in args)
        assert fn(None, *good) == -1, name
        assert L.gpd_hip_last_error() == text, (name, L.gpd_hip_last_error())
        if args is not None:
            assert fn(ctx, *args) == -1, name
            assert L.gpd_hip_last_error() == text, (name, L.gpd_hip_last_error())
