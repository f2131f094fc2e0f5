"""The host side of the growable resident sets: exported symbols with their ctypes signatures, the public struct sizes, and the
train tool's argument parser.  No device is needed."""
import ctypes as C

import pytest

from gpd_amd import api, hostlib, train

POOL_ENTRIES = {
    "gpd_hip_train_reserve": [C.c_void_p, C.c_int, C.c_int],
    "gpd_hip_train_count": [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "gpd_hip_train_append_data": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int],
    "gpd_hip_train_get_data": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "gpd_hip_train_reorder": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p],
    "gpd_hip_train_append_view": [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(api.LabelViewJob)],
}


def test_the_pool_entries_are_exported_with_their_signatures():
    L = api.lib()
    for name, argtypes in POOL_ENTRIES.items():
        assert name in api.EXPORTS, name
        f = getattr(L, name)
        assert list(f.argtypes) == argtypes, name
        assert f.restype is C.c_int, name
    for method in ("reserve", "count", "append_data", "get_data", "reorder", "append_view"):
        assert callable(getattr(api.Trainer, method)), method


def test_null_arguments_are_refused_without_a_device():
    L = api.lib()
    n = C.c_int(7)
    assert L.gpd_hip_train_reserve(None, 0, 4) == -1
    assert L.gpd_hip_train_count(None, 0, C.byref(n), None) == -1 and n.value == 7
    assert L.gpd_hip_train_append_data(None, 0, None, None, 0) == -1
    assert L.gpd_hip_train_get_data(None, 0, 0, 0, None, None) == -1
    assert L.gpd_hip_train_reorder(None, 0, 0, 0, None) == -1
    assert L.gpd_hip_train_append_view(None, 0, None, None) == -1
    assert b"gpd_hip_train_append_view" in L.gpd_hip_last_error()


def test_the_host_mirror_exports_generate_data():
    f = hostlib.lib().gpd_host_generate_data
    assert callable(hostlib.generate_data)
    f.argtypes = [C.c_char_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    f.restype = C.c_int
    assert f(None, None, None, None) == -1  # nothing to do: refused before any work


def test_the_public_struct_sizes_are_unchanged():
    # gpd_label_view_job: 8 pointers and 13 32-bit fields, an int64, four floats, the padding of the x86-64 ABI
    assert C.sizeof(api.LabelViewJob) == 136
    assert api.lib().gpd_hip_sizeof_label_view_job() == 136
    # gpd_train_params: two ints and six doubles
    assert C.sizeof(api.TrainParams) == 56
    # gpd_train_recipe: two ints, a double, two ints, two doubles, 2 x 8 doubles
    assert C.sizeof(api.TrainRecipe) == 168
    assert api.lib().gpd_hip_sizeof_train_recipe() == 168


def test_generate_and_train_dir_exclude_each_other(capsys):
    a = train.parse_args(["--generate", "generate_data.cfg", "--epochs", "1", "--out", "net"])
    assert a.generate == "generate_data.cfg" and a.train_dir is None
    a = train.parse_args(["data", "--out", "net"])
    assert a.train_dir == "data" and a.generate is None
    for argv in (["data", "--generate", "generate_data.cfg", "--out", "net"],
                 ["--generate", "generate_data.cfg", "--test", "data", "--out", "net"],
                 ["--generate", "generate_data.cfg", "--recipe", "caffe", "data", "--out", "net"],
                 ["--out", "net"]):
        with pytest.raises(SystemExit) as e:
            train.parse_args(argv)
        assert e.value.code == 2, argv
    assert "--generate" in capsys.readouterr().err


def test_the_configuration_reader(tmp_path):
    cfg = tmp_path / "generate_data.cfg"
    cfg.write_text("# a comment\nimage_num_channels = 3   # trailing\nhip_device=0\n\ndata_root = /somewhere/\n")
    v = train.config_values(str(cfg))
    assert v == {"image_num_channels": "3", "hip_device": "0", "data_root": "/somewhere/"}
