"""The shape-general LeNet route (gpd_hip_set_lenet_net, lenet_net.hip) at the edges tests/test_gpu_lenet_net.py does not reach.
Every comparison is an equality: against the k-ascending f32 fmaf chain network of lenet_net_ref.py (oracle.conv_generic, none of
the code under test) or against another entry of the library.  No tolerance anywhere; the counted conditions on the reference
inputs are asserted on the CPU (tests/test_lenet_net.py).

  a. edge shapes F, G, H, I (lenet_net_ref.EDGE_SHAPES): 12 channels, conv2 as one odd-k chunk, a dense K that is no multiple
     of 4 (the X address clamp, the never-written padding of h1 / h2), widths of 1, widths that are exact tile multiples;
  b. batch edges: the three image tilings of the dense kernel (n <= 32, <= 64, above), a second workgroup in x (n > 128) and of
     the logits kernel (n > 256), the scratch growing on the way — activations, not only scores;
  c. hostile magnitudes: subnormal weights, products, sums and planes, values above 2^90, wide spans inside one chain, zero rows;
  d. one context, several shapes, and the stock route in between;
  e. two contexts with two shapes on one device, alternately and from two threads;
  f. the entries that reach lenet_forward with a lane's own scratch: detect_batch over both lanes, detect_batch_multi,
     detect_sharded, detect_sis, replay;
  g. presizing: gpd_hip_reserve and the batch entry size the GENERAL route's scratch once, before the first cloud.
"""
import threading

import numpy as np
import pytest

import lenet_net_ref as R
import lenet_torch_ref as ltr
from gpd_amd import api, synth
from test_gpu_lenet_net import DEBUG, _check_against_chain, _ctx

pytestmark = pytest.mark.gpu
BATCH_EDGES = (31, 32, 33, 63, 64, 65, 127, 128, 129, 257)


# ---- a. edge shapes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.EDGE_SHAPES))
def test_edge_shapes_are_the_chain_bit_for_bit(name):
    C, F1, F2, H1, H2 = R.EDGE_SHAPES[name]
    ctx = _ctx(C)
    try:
        for relu in (True, False) if name in "FG" else (True,):
            shape = ctx.set_lenet_net(R.state(name), R.INPUT_SCALE, conv_relu=relu)
            assert shape.as_tuple() == R.EDGE_SHAPES[name]
            info = ctx.lenet_net_info()
            assert info["scratch_bytes_per_image"] == 4 * (F1 * 784 + F2 * 144 + (H1 + 3) // 4 * 4 + (H2 + 3) // 4 * 4 + 2)
            assert info["macs_per_image"] == F1 * 3136 * C * 25 + F2 * 576 * F1 * 25 + F2 * 144 * H1 + H1 * (H2 or 2) + H2 * 2
            want = R.chain(name, False, relu)
            for n in (1, 35):
                _check_against_chain(ctx, name, want, n, "%s relu = %d" % (name, relu))
    finally:
        ctx.close()


# ---- b. batch edges ---------------------------------------------------------------------------------------------------------
def test_batch_edges_on_one_context():
    """Shape F (fc2 with K = 130: the clamp and the padding at every tiling); the sizes ascend, so the scratch is re-sized at 31, 63,
    127 and 257 and re-used in between; then one image in the scratch of 257"""
    name = "F"
    ctx = _ctx(R.EDGE_SHAPES[name][0])
    try:
        ctx.set_lenet_net(R.state(name))
        want = R.chain(name)
        for n in BATCH_EDGES + (1,):
            _check_against_chain(ctx, name, want, n, "F batch edge")
    finally:
        ctx.close()


# ---- c. hostile magnitudes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False], ids=["conv_relu", "no_conv_relu"])
def test_hostile_magnitudes_are_the_chain_bit_for_bit(relu):
    """lenet_net_ref.hostile_state("F"): what it contains is asserted by test_lenet_net.py::test_hostile_set_has_what_it_is_for.
    Values are compared (array_equal), not bytes: the u8 loader's skip of blank steps may change the sign of a zero sum."""
    name = "F"
    img = R.hostile_images(name)
    want = R.hostile_chain(name, relu)
    ctx = _ctx(R.EDGE_SHAPES[name][0])
    try:
        ctx.set_lenet_net(R.hostile_state(name), R.INPUT_SCALE, conv_relu=relu)
        # measured before anything is asserted: where a difference sits (a flushing build or unit shows as differences on
        # subnormal values only)
        ctx.score(img)
        for which, key in DEBUG:
            got, ref = ctx.lenet_net_debug(which, len(img)), want[key]
            diff = got != ref
            tiny = np.abs(ref) < np.float32(2.0 ** -126)
            print("hostile relu = %d %s: %d subnormals expected, %d on the device; %d of %d values differ, %d of them where the chain "
                  "is subnormal or zero" % (relu, key, R.subnormals(ref), R.subnormals(got), int(diff.sum()), diff.size,
                                            int((diff & tiny).sum())))
        for n in (len(img), 1):
            _check_against_chain(ctx, name, want, n, "hostile relu = %d" % relu, imgs=img)
    finally:
        ctx.close()


# ---- d. one context, several shapes ----------------------------------------------------------------------------------------
def test_one_context_takes_shape_after_shape():
    C = 1
    stock_w = ltr.eigen_weights(C)
    img35 = R.images("B", 35)
    fresh = _ctx(C)
    try:
        fresh.set_lenet_weights(stock_w)
        fresh.set_lenet_conv_relu(True)  # set_lenet_net switches the conv ReLUs on, and set_lenet_weights keeps the setting
        stock_scores = fresh.score(img35)
    finally:
        fresh.close()
    ctx = _ctx(C)
    try:
        for name, n in (("B", 35), ("E", 3), ("I", 35), ("B", 35)):
            shape = ctx.set_lenet_net(R.state(name))
            assert shape.as_tuple() == R.ALL_SHAPES[name]
            F1, F2, H1, H2 = R.ALL_SHAPES[name][1:]
            info = ctx.lenet_net_info()
            assert info["scratch_bytes_per_image"] == 4 * (F1 * 784 + F2 * 144 + (H1 + 3) // 4 * 4 + (H2 + 3) // 4 * 4 + 2)
            assert info["macs_per_image"] == F1 * 3136 * C * 25 + F2 * 576 * F1 * 25 + F2 * 144 * H1 + H1 * (H2 or 2) + H2 * 2
            with pytest.raises(api.GpdHipError, match="general route"):
                ctx.lenet_net_debug(4, 1)  # the scratch of the previous shape is gone, nothing ran on the new one
            _check_against_chain(ctx, name, R.chain(name), n, "%s after another shape" % name)
            with pytest.raises(api.GpdHipError, match="exceeds the first chunk"):
                ctx.lenet_net_debug(4, 2 * n + 8)  # the scratch holds n and a quarter more
            if not H2:
                with pytest.raises(api.GpdHipError, match="without fc2"):
                    ctx.lenet_net_debug(3, 1)
        general = ctx.score(img35)
        ctx.set_lenet_weights(stock_w)  # back to the stock route ...
        assert np.array_equal(ctx.score(img35), stock_scores)
        with pytest.raises(api.GpdHipError):
            ctx.lenet_net_info()
        ctx.set_lenet_net(R.state("B"))  # ... and to the general one: bits unchanged
        again = _check_against_chain(ctx, "B", R.chain("B"), 35, "B after the stock route")
        assert general.tobytes() == again.tobytes()
    finally:
        ctx.close()


# ---- e. two contexts, two shapes, one device -----------------------------------------------------------------------------------
def test_two_contexts_with_two_shapes_alternately():
    """A and G are both C = 3.  G is installed first and A second: whatever gpd_hip_set_lenet_net sets per FUNCTION (the dynamic
    LDS attribute of the conv kernels) is then A's, the smaller one, when G scores."""
    ctxs = {}
    try:
        for name in ("G", "A"):
            ctxs[name] = _ctx(3)
            ctxs[name].set_lenet_net(R.state(name))
        for rnd, n in enumerate((35, 1, 65, 129, 33, 257)):
            for name in ("A", "G") if rnd % 2 else ("G", "A"):
                if rnd < 2:
                    _check_against_chain(ctxs[name], name, R.chain(name), n, "%s alternately, round %d" % (name, rnd))
                else:
                    sc = ctxs[name].score(R.images(name, n))
                    assert np.array_equal(sc, R.chain(name)["score"][np.arange(n) % 35]), (name, rnd, n)
                    assert np.array_equal(ctxs[name].lenet_net_debug(4, n), R.chain(name)["logits"][np.arange(n) % 35]), (name, rnd, n)
    finally:
        for c in ctxs.values():
            c.close()


def test_two_contexts_with_two_shapes_from_two_threads():
    """As test_gpu_lenet_stress.py::test_two_contexts_from_two_threads: each thread its own context, 40 scoring calls each at the
    batch edges, every score equal to the chain"""
    errors = []
    wants = {name: R.chain(name)["score"] for name in ("A", "G")}  # computed before the threads start
    start = threading.Barrier(2)

    def worker(name, seed):
        try:
            rng = np.random.RandomState(seed)
            ctx = _ctx(3)
            try:
                ctx.set_lenet_net(R.state(name))
                start.wait(timeout=60)
                for it in range(40):
                    n = int(BATCH_EDGES[rng.randint(len(BATCH_EDGES))])
                    first = int(rng.randint(35))
                    idx = (first + np.arange(n)) % 35
                    got = ctx.score(R.images(name, 35)[idx])
                    assert np.array_equal(got, wants[name][idx]), (name, it, n)
            finally:
                ctx.close()
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))
            start.abort()

    th = [threading.Thread(target=worker, args=a) for a in (("A", 7), ("G", 8))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


# ---- f. the entries ------------------------------------------------------------------------------------------------------------
NAME = "A"
CLOUD_SEEDS = (5, 6, 7, 8)


def _net_ctx():
    ctx = _ctx(R.SHAPES[NAME][0])
    ctx.set_lenet_net(R.state(NAME))
    return ctx


def _upload(ctx, cl):
    ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])


@pytest.fixture(scope="module")
def scored_clouds(oracle_mod):
    """Four small clouds; per cloud the scores of its candidates by images + score on a fresh context, which equal the chain
    network on those images.  Shared and left unchanged."""
    out = []
    for seed in CLOUD_SEEDS:
        cl = synth.make_cloud(seed, 2000)
        si = synth.sample_indices(cl, 30)
        ctx = _net_ctx()
        try:
            _upload(ctx, cl)
            hands, n_cand = ctx.detect(si)
            img, cand = ctx.images(hands.copy())
            want = ctx.score(img)
        finally:
            ctx.close()
        assert len(cand) == n_cand >= 20
        ref = R.chain_batch(oracle_mod, R.SHAPES[NAME], R.route_arrays(NAME)[1], img)["score"]
        assert np.array_equal(want, ref), seed
        want.setflags(write=False)
        out.append((cl, si, want))
    return out


def test_detect_batch_scores_on_both_lanes(scored_clouds):
    clouds, samples = [c for c, _, _ in scored_clouds], [s for _, s, _ in scored_clouds]
    ctx = _net_ctx()
    try:
        for _ in range(2):  # the second batch runs in the scratch the first one left
            got = ctx.detect_batch(clouds, samples, 0)
            assert len(got) == 4
            for (hands, _, nc, _), (_, _, want) in zip(got, scored_clouds):
                assert nc == len(want) == len(hands) and np.array_equal(hands["score"], want)
    finally:
        ctx.close()


def test_detect_batch_multi_scores_on_every_context(scored_clouds):
    clouds, samples = [c for c, _, _ in scored_clouds], [s for _, s, _ in scored_clouds]
    ctxs = [_net_ctx() for _ in range(2)]
    try:
        got = ctxs[0].detect_batch_multi(ctxs[1:], clouds, samples, 0)
        assert len(got) == 4
        for (hands, _, nc, _), (_, _, want) in zip(got, scored_clouds):
            assert nc == len(want) == len(hands) and np.array_equal(hands["score"], want)
    finally:
        for c in ctxs:
            c.close()


def test_detect_sharded_scores_like_the_single_call(scored_clouds):
    cl, si, want = scored_clouds[0]
    ctxs = [_net_ctx() for _ in range(2)]
    try:
        _upload(ctxs[0], cl)
        single, _, nc = ctxs[0].detect_select(si, 0)
        single = single.copy()
        assert nc == len(want) and np.array_equal(single["score"], want)
        got, info = ctxs[0].detect_sharded(ctxs[1:], cl, si)
        assert all(i[1] > 0 for i in info) and sum(i[1] for i in info) == nc
        assert np.array_equal(got["score"], want)
        assert got.tobytes() == single.tobytes()
    finally:
        for c in ctxs:
            c.close()


def test_detect_sis_reports_the_scores_of_its_hands(scored_clouds):
    """One round after the initial pass; every candidate comes back (min_score below any score).  The hands it returns, put back
    into their sets and handed to score_given, get the scores it reported."""
    cl, si, want = scored_clouds[1]
    lo, hi = cl["xyz"].min(axis=0) - 0.5, cl["xyz"].max(axis=0) + 0.5
    ctx = _net_ctx()
    try:
        _upload(ctx, cl)
        got = ctx.detect_sis(si, 1, 10, min_score=-3.0e38, workspace=(lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]), seed=3)
        hands = got["hands"]
        assert got["rounds_run"] == 1 and got["num_candidates"] == len(hands) >= len(want)
        sets, slots = hands["set_index"], hands["slot"]
        assert sets.min() >= 0 and sets.max() < got["num_sets"] and 0 <= slots.min() and slots.max() < ctx.n_slots
        given = np.zeros((got["num_sets"], ctx.n_slots), api.HAND_DTYPE)
        given[sets, slots] = hands
        first = np.unique(sets, return_index=True)[1]
        given["sample"][sets[first], 0] = hands["sample"][first]  # a set's sample is read from slot 0, valid or not
        assert int(given["valid"].astype(bool).sum()) == len(hands)
        scored, scores, cand, _ = ctx.score_given(given)
        assert np.array_equal(scored[sets, slots]["score"], hands["score"])
        assert np.array_equal(np.sort(scores), np.sort(hands["score"]))
        assert len(np.unique(hands["score"])) > len(hands) // 2
    finally:
        ctx.close()


def test_replay_scores_like_detect(scored_clouds):
    cl, si, want = scored_clouds[2]
    ctx = _net_ctx()
    try:
        _upload(ctx, cl)
        hands, n_cand = ctx.detect(si)
        hands = hands.copy()
        assert n_cand == len(want) and np.array_equal(hands["score"][hands["valid"].astype(bool)], want)
        ctx.replay(3)
        ctx.replay(2)
        _, lenet_ms, launches, sc = ctx.replay_times(n_scores=n_cand)
        assert launches == 2 and lenet_ms > 0 and np.array_equal(sc, want)
        ms = ctx.replay_kernel_ms()
        assert len(ms) == 4 and all(x > 0 for x in ms[:3]), ms  # conv1, conv2, fc1 between the route's three events
    finally:
        ctx.close()


# ---- g. presizing --------------------------------------------------------------------------------------------------------------
def test_reserve_then_batch_allocates_nothing_on_the_general_route():
    """The counterpart of test_gpu_resident.py::test_reserve_then_batch_allocates_nothing: after set_lenet_net, gpd_hip_reserve
    sizes both lanes once — the general route's scratch included — and a batch within those sizes books no buffer growth
    (`allocs`) beyond what the same clouds cause on the stock route (a list-capacity retry of the search, which has nothing to do
    with the network).  Without the reservation the batch entry sizes the lanes itself, booked on the first cloud only."""
    C = R.SHAPES[NAME][0]
    clouds = [synth.make_cloud(900 + cid, 2000 + 500 * cid) for cid in range(3)]
    samples = [synth.sample_indices(cl, 30 + 5 * cid) for cid, cl in enumerate(clouds)]
    sizes = dict(max_points=max(len(cl["xyz"]) for cl in clouds), max_cams=1, max_samples=max(len(s) for s in samples))
    results = {}
    for reserve in (True, False):
        net, stock = _net_ctx(), _ctx(C)
        try:
            stock.set_lenet_torch(ltr.state(C))
            allocs = {}
            for label, c in (("general", net), ("stock", stock)):
                if reserve:
                    c.reserve(**sizes)
                got = c.detect_batch(clouds, samples, 0)
                allocs[label] = [a for _, a in c.last_batch_timeline]
                c.detect_batch(clouds, samples, 0)  # a second batch of the same sizes: nothing grows either way
                allocs[label + ", second batch"] = [a for _, a in c.last_batch_timeline]
                results[label, reserve] = [(nc, h["score"].copy()) for h, _, nc, _ in got]
            print("reserve = %d: allocs per cloud %s" % (reserve, allocs))
            assert all(nc >= 20 for nc, _ in results["general", reserve])
            assert allocs["stock, second batch"] == [0, 0, 0] and allocs["general, second batch"] == [0, 0, 0], allocs
            if reserve:
                assert allocs["general"] == allocs["stock"], allocs
            else:
                assert allocs["general"][0] > 0 and allocs["stock"][0] > 0, allocs
                assert allocs["general"][1:] == allocs["stock"][1:], allocs
        finally:
            net.close()
            stock.close()
    # the reservation changes no score, and the two networks are different networks on the same candidates
    for (nc_a, sa), (nc_b, sb), (nc_s, ss) in zip(results["general", True], results["general", False], results["stock", True]):
        assert nc_a == nc_b == nc_s and np.array_equal(sa, sb) and np.abs(sa - ss).max() > 1e-3
