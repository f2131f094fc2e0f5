"""Every refusal of the trainer's table entries (set_state, get_state, get_solver_state, set_solver_state, gradients, apply, in
their 8-tensor and 10-tensor forms) and of its resident-set entries: the return code and the full text of
gpd_hip_last_error(), written out here, and after each refusal the trainer as it was — parameters, solver buffers and update
count, both sets' counts and the training set's bytes.

The smallest trainer creation admits: one channel, every width 1 (gpd_hip_lenet_shape_check's lower limits), max_batch 2, three
resident images; once without a third dense layer (eight tensors) and once with it at width 1 (ten).  Nothing heavier than a copy
is launched.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -4
NAMES = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias")
TEN = "%s: the trainer's network has a third dense layer and ten tensors; use the gpd_hip_train_net_ entry"


class _Rig:
    """The trainer of widths (1, 1, 1, H2) with a state, solver buffers and a count that are not zero, and three images."""

    def __init__(self, H2):
        from gpd_amd import api
        self.api, self.L = api, api.lib()
        self.ctx = api.Context(api.default_params(1))
        self.t = api.Trainer(self.ctx, api.train_default_params(1, 2), None, shape=(1, 1, 1, H2))
        self.h, self.nt = self.t._h, 10 if H2 else 8
        rng = np.random.default_rng(7 + H2)
        self.state = api.init_state(1, 11, shape=(1, 1, 1, H2))
        self.t.set_state(self.state)
        self.t.set_solver_state(dict(count=5, m={k: rng.standard_normal(v.shape).astype(np.float32) for k, v in self.state.items()},
                                     v={k: rng.random(v.shape).astype(np.float32) for k, v in self.state.items()}))
        self.img = rng.integers(0, 256, (3, 60, 60, 1), dtype=np.uint8)
        self.lab = np.array([0, 1, 1], np.uint8)
        self.t.set_data(self.img, self.lab)
        # the forms that serve this trainer; the 8-tensor form of a ten-tensor trainer has a test of its own
        self.forms = ("gpd_hip_train_net_",) if H2 else ("gpd_hip_train_", "gpd_hip_train_net_")
        self.before = self.snapshot()

    def close(self):
        self.t.close()
        self.ctx.close()

    def snapshot(self):
        s = self.t.get_solver_state()
        parts = [a.tobytes() for a in self.t.get_state().values()] + [a.tobytes() for b in (s["m"], s["v"]) for a in b.values()]
        img, lab = self.t.get_data()
        return parts, s["count"], self.t.count(0), self.t.count(1), img.tobytes(), lab.tobytes()

    def arrays(self):
        """a table's worth of finite arrays in tensor order"""
        return [np.full(v.shape, 0.25, np.float32) for v in self.state.values()]

    def refused(self, rc, text, name, *args):
        """entry `name` returns rc with exactly this text, and the trainer is as it was"""
        got = getattr(self.L, name)(self.h, *args)
        said = self.L.gpd_hip_last_error().decode()
        assert (got, said) == (rc, text), (name, got, said)
        assert self.snapshot() == self.before, name


def table(arrs, null=None):
    """the pointer table of these arrays, which live as long as it does; slot `null` empty"""
    t = (C.c_void_p * 10)()
    for i, a in enumerate(arrs):
        t[i] = None if i == null else a.ctypes.data
    t.arrays = arrs
    return t


@pytest.fixture(scope="module", params=[0, 1], ids=["eight_tensors", "ten_tensors"])
def rig(request):
    r = _Rig(request.param)
    yield r
    r.close()


def test_a_null_table(rig):
    idx, loss, n = np.zeros(1, np.int32), C.c_float(0), C.c_longlong(0)
    ok = table(rig.arrays())
    for f in rig.forms:
        rig.refused(INVALID, f + "set_state: null argument", f + "set_state", None)
        rig.refused(INVALID, f + "get_state: null argument", f + "get_state", None)
        rig.refused(INVALID, f + "apply: null argument", f + "apply", None)
        rig.refused(INVALID, f + "gradients: null argument", f + "gradients", idx.ctypes.data, 1, None, C.byref(loss))
        rig.refused(INVALID, f + "gradients: null argument", f + "gradients", idx.ctypes.data, 1, ok, None)
        rig.refused(INVALID, f + "gradients: null argument", f + "gradients", None, 1, ok, C.byref(loss))
        rig.refused(INVALID, f + "get_solver_state: null argument", f + "get_solver_state", None, ok, C.byref(n))
        rig.refused(INVALID, f + "get_solver_state: null argument", f + "get_solver_state", ok, None, C.byref(n))  # Adam: v is needed
        rig.refused(INVALID, f + "get_solver_state: null argument", f + "get_solver_state", ok, ok, None)
        rig.refused(INVALID, f + "set_solver_state: null argument or a negative count", f + "set_solver_state", None, ok, 5)
        rig.refused(INVALID, f + "set_solver_state: null argument or a negative count", f + "set_solver_state", ok, None, 5)


def test_a_null_slot_first_and_last(rig):
    idx, loss, n = np.zeros(1, np.int32), C.c_float(0), C.c_longlong(0)
    arrs = rig.arrays()
    ok = table(arrs)
    for f in rig.forms:
        for i in (0, rig.nt - 1):
            bad = table(arrs, null=i)
            rig.refused(INVALID, f + "set_state: %s is null or holds a non-finite value" % NAMES[i], f + "set_state", bad)
            rig.refused(INVALID, f + "get_state: tensor %d is null" % i, f + "get_state", bad)
            rig.refused(INVALID, f + "apply: tensor %d is null or holds a non-finite value" % i, f + "apply", bad)
            rig.refused(INVALID, f + "gradients: tensor %d is null" % i, f + "gradients", idx.ctypes.data, 1, bad, C.byref(loss))
            rig.refused(INVALID, f + "get_solver_state: tensor %d is null" % i, f + "get_solver_state", bad, ok, C.byref(n))
            rig.refused(INVALID, f + "get_solver_state: tensor %d is null" % i, f + "get_solver_state", ok, bad, C.byref(n))
            rig.refused(INVALID, f + "set_solver_state: buffer 0, tensor %d is null or holds a non-finite value" % i, f + "set_solver_state", bad, ok, 5)
            rig.refused(INVALID, f + "set_solver_state: buffer 1, tensor %d is null or holds a non-finite value" % i, f + "set_solver_state", ok, bad, 5)
    assert n.value == 0  # no refused getter wrote the count


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_value_in_the_first_and_in_the_last_tensor(rig, value):
    ok = table(rig.arrays())
    for f in rig.forms:
        for i in (0, rig.nt - 1):
            arrs = rig.arrays()
            arrs[i].reshape(-1)[-1] = value
            bad = table(arrs)
            rig.refused(INVALID, f + "set_state: %s is null or holds a non-finite value" % NAMES[i], f + "set_state", bad)
            rig.refused(INVALID, f + "apply: tensor %d is null or holds a non-finite value" % i, f + "apply", bad)
            rig.refused(INVALID, f + "set_solver_state: buffer 0, tensor %d is null or holds a non-finite value" % i, f + "set_solver_state", bad, ok, 5)
            rig.refused(INVALID, f + "set_solver_state: buffer 1, tensor %d is null or holds a non-finite value" % i, f + "set_solver_state", ok, bad, 5)


def test_the_first_bad_tensor_is_the_one_named(rig):
    """two bad tensors: the lower one is reported, and a bad m goes before a bad v"""
    arrs = rig.arrays()
    arrs[2][...] = np.nan
    arrs[5][...] = np.nan
    bad, ok = table(arrs, null=6), table(rig.arrays())
    for f in rig.forms:
        rig.refused(INVALID, f + "set_state: conv2.weight is null or holds a non-finite value", f + "set_state", bad)
        rig.refused(INVALID, f + "apply: tensor 2 is null or holds a non-finite value", f + "apply", bad)
        rig.refused(INVALID, f + "get_state: tensor 6 is null", f + "get_state", bad)
        rig.refused(INVALID, f + "set_solver_state: buffer 0, tensor 2 is null or holds a non-finite value", f + "set_solver_state", bad, bad, 5)
        rig.refused(INVALID, f + "set_solver_state: buffer 1, tensor 2 is null or holds a non-finite value", f + "set_solver_state", ok, bad, 5)


def test_a_negative_solver_count(rig):
    ok = table(rig.arrays())
    for f in rig.forms:
        rig.refused(INVALID, f + "set_solver_state: null argument or a negative count", f + "set_solver_state", ok, ok, -1)


def test_a_table_of_eight_on_a_trainer_of_ten_tensors(rig):
    if rig.nt == 8:  # served: the forms above are both of them
        assert rig.forms == ("gpd_hip_train_", "gpd_hip_train_net_")
        return
    idx, loss, n = np.zeros(1, np.int32), C.c_float(0), C.c_longlong(0)
    ok = table(rig.arrays())
    f = "gpd_hip_train_"
    rig.refused(STATE, TEN % (f + "set_state"), f + "set_state", ok)
    rig.refused(STATE, TEN % (f + "get_state"), f + "get_state", ok)
    rig.refused(STATE, TEN % (f + "apply"), f + "apply", ok)
    rig.refused(STATE, TEN % (f + "gradients"), f + "gradients", idx.ctypes.data, 1, ok, C.byref(loss))
    rig.refused(STATE, TEN % (f + "get_solver_state"), f + "get_solver_state", ok, ok, C.byref(n))
    rig.refused(STATE, TEN % (f + "set_solver_state"), f + "set_solver_state", ok, ok, 5)
    # ... whatever else is wrong with the call: the form is refused first
    rig.refused(STATE, TEN % (f + "set_state"), f + "set_state", None)
    rig.refused(STATE, TEN % (f + "set_solver_state"), f + "set_solver_state", None, None, -1)


def test_the_resident_sets(rig):
    img, lab = rig.img, rig.lab
    ip, lp = img.ctypes.data, lab.ctypes.data
    n, cap, k = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    order = np.array([2, 0, 1], np.int32)
    job = rig.api.LabelViewJob()
    logits = np.zeros((3, 2), np.float32)
    # which = 2
    rig.refused(INVALID, "gpd_hip_train_set_data: bad argument", "gpd_hip_train_set_data", 2, ip, lp, 3)
    rig.refused(INVALID, "gpd_hip_train_reserve: bad argument", "gpd_hip_train_reserve", 2, 8)
    rig.refused(INVALID, "gpd_hip_train_count: bad argument", "gpd_hip_train_count", 2, C.byref(n), C.byref(cap))
    rig.refused(INVALID, "gpd_hip_train_append_data: bad argument", "gpd_hip_train_append_data", 2, ip, lp, 3)
    rig.refused(INVALID, "gpd_hip_train_get_data: bad argument, or a range outside the 0 images of the set", "gpd_hip_train_get_data", 2, 0, 1, ip, lp)
    rig.refused(INVALID, "gpd_hip_train_reorder: bad argument, or a range outside the 0 images of the set", "gpd_hip_train_reorder", 2, 0, 3,
                order.ctypes.data)
    rig.refused(INVALID, "gpd_hip_train_append_view: bad argument", "gpd_hip_train_append_view", 2, rig.ctx._h, C.byref(job))
    rig.refused(INVALID, "gpd_hip_train_eval: bad argument", "gpd_hip_train_eval", 2, None, 3, logits.ctypes.data, C.byref(k))
    rig.refused(INVALID, "gpd_hip_train_set_data: bad argument", "gpd_hip_train_set_data", -1, ip, lp, 3)
    assert (n.value, cap.value, k.value) == (-7, -7, -7)
    # a label of 2
    two = np.array([0, 2, 1], np.uint8)
    for which in (0, 1):
        rig.refused(INVALID, "gpd_hip_train_set_data: label 2 of image 1 (0 or 1)", "gpd_hip_train_set_data", which, ip, two.ctypes.data, 3)
        rig.refused(INVALID, "gpd_hip_train_append_data: label 2 of image 1 (0 or 1)", "gpd_hip_train_append_data", which, ip, two.ctypes.data, 3)
    high = np.array([255, 0, 1], np.uint8)
    rig.refused(INVALID, "gpd_hip_train_set_data: label 255 of image 0 (0 or 1)", "gpd_hip_train_set_data", 0, ip, high.ctypes.data, 3)
    # a range past the set: the training set holds three images, the test set none
    out_i, out_l = np.zeros_like(img), np.zeros_like(lab)
    for first, count in ((2, 2), (4, 0), (0, 4), (-1, 1), (0x7fffffff, 0x7fffffff)):
        rig.refused(INVALID, "gpd_hip_train_get_data: bad argument, or a range outside the 3 images of the set", "gpd_hip_train_get_data", 0, first,
                    count, out_i.ctypes.data, out_l.ctypes.data)
        rig.refused(INVALID, "gpd_hip_train_reorder: bad argument, or a range outside the 3 images of the set", "gpd_hip_train_reorder", 0, first,
                    count, order.ctypes.data)
    rig.refused(INVALID, "gpd_hip_train_get_data: bad argument, or a range outside the 0 images of the set", "gpd_hip_train_get_data", 1, 0, 1,
                out_i.ctypes.data, out_l.ctypes.data)
    rig.refused(INVALID, "gpd_hip_train_reorder: bad argument, or a range outside the 0 images of the set", "gpd_hip_train_reorder", 1, 0, 1,
                order.ctypes.data)
    assert not out_i.any() and not out_l.any()
    # an order that is no permutation
    for bad, text in (([0, 0, 1], "order[1] = 0"), ([2, 1, 3], "order[2] = 3"), ([-1, 1, 2], "order[0] = -1")):
        o = np.array(bad, np.int32)
        rig.refused(INVALID, "gpd_hip_train_reorder: %s: not a permutation of 0 .. 2" % text, "gpd_hip_train_reorder", 0, 0, 3, o.ctypes.data)
    o = np.array([1, 1], np.int32)
    rig.refused(INVALID, "gpd_hip_train_reorder: order[1] = 1: not a permutation of 0 .. 1", "gpd_hip_train_reorder", 0, 1, 2, o.ctypes.data)


def test_the_entries_still_serve_beside_the_refusals(rig):
    """what is refused above goes through when it is right, in every form that serves the trainer"""
    n = C.c_longlong(0)
    for f in rig.forms:
        got = [np.zeros(v.shape, np.float32) for v in rig.state.values()]
        assert getattr(rig.L, f + "get_state")(rig.h, table(got)) == 0
        assert [a.tobytes() for a in got] == rig.before[0][:rig.nt]
        m, v = rig.arrays(), rig.arrays()
        assert getattr(rig.L, f + "get_solver_state")(rig.h, table(m), table(v), C.byref(n)) == 0
        assert n.value == 5 and [a.tobytes() for a in m + v] == rig.before[0][rig.nt:]
    rig.t.reorder(0, [2, 0, 1])
    img, lab = rig.t.get_data()
    assert np.array_equal(img, rig.img[[2, 0, 1]]) and np.array_equal(lab, rig.lab[[2, 0, 1]])
    rig.t.reorder(0, [1, 2, 0])  # and back
    assert rig.snapshot() == rig.before
