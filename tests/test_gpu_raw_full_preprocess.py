"""The last stretch of CandidatesGenerator::preprocessPointCloud inside a RAW job of gpd_hip_detect_batch: refineNormals,
sampleAbovePlane and subsample resident on the device (gpd_detect_job.refine_normals_k / sample_above_plane / num_draws).

The reference of every comparison is the stepwise route through the single-call entries — gpd_hip_preprocess_cloud, upload,
gpd_hip_estimate_normals, gpd_hip_refine_normals, gpd_hip_sample_above_plane, then gpd_hip_detect_select at the sample indices
the numpy restatement of the draw stream picks — each of which is proven against the oracle / numpy restatements in
test_gpu_preprocess.py, test_gpu_refine_normals.py and test_gpu_plane_fit.py.  The raw job is never its own reference."""
import ctypes as C
import os

import numpy as np
import pytest

from gpd_amd import api, synth
from pyref_sample import dense_fisher_yates as _dense_fisher_yates, with_repetition as _with_repetition

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
WS = np.array([-0.4, 0.4, -0.4, 0.4, -1.0, 1.0])
CELL, RADIUS = 0.003, 0.03


synth_scan = synth.raw_scan


def table_mug_scan():
    xyz = np.load(os.path.join(GOLD, "table_mug_xyz.npz"))["xyz"].astype(np.float32)
    return dict(xyz=xyz, cam_source=np.ones((1, len(xyz)), np.int32), view_points=np.zeros((1, 3)))


def flat_scan(seed=5, n=20000):
    """A table and nothing on it: every point within a millimetre of one plane, so no point is off the fitted plane and
    sampleAbovePlane reports "plane fit failed"."""
    rng = np.random.RandomState(seed)
    xyz = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), -0.8 + rng.uniform(-1e-3, 1e-3, n)], 1).astype(np.float32)
    return dict(xyz=xyz, cam_source=np.ones((1, n), np.int32), view_points=np.zeros((1, 3)))


TWO_WS = np.array([-0.02, 0.02, -0.02, 0.02, -1.0, 1.0])


def two_point_scan():
    """The flat table with a hole around the origin and two points a centimetre apart in it: TWO_WS keeps those two."""
    xyz = flat_scan(6, 2000)["xyz"]
    xyz = xyz[(np.abs(xyz[:, 0]) > 0.03) | (np.abs(xyz[:, 1]) > 0.03)]
    xyz = np.concatenate([xyz[:1000], np.array([[0.0, 0.0, -0.8], [0.01, 0.005, -0.8]], np.float32), xyz[1000:]])
    return dict(xyz=np.ascontiguousarray(xyz), cam_source=np.ones((1, len(xyz)), np.int32), view_points=np.zeros((1, 3)))


def spec(scan, ws=None, sm=None, k=0, plane=False, draws=0, seed=0):
    return dict(scan=scan, ws=ws, sm=sm, k=k, plane=plane, draws=draws, seed=seed)


def _inside(p, ws):
    return (p[:, 0] > ws[0]) & (p[:, 0] < ws[1]) & (p[:, 1] > ws[2]) & (p[:, 1] < ws[3]) & (p[:, 2] > ws[4]) & (p[:, 2] < ws[5])


def stepwise(ctx, s):
    """One spec through the single calls of the parent commit, every cloud-sized array crossing PCIe in between."""
    scan = s["scan"]
    vox, cam, _, _ = ctx.preprocess_cloud(scan["xyz"], scan["cam_source"], s["ws"], CELL)
    ctx.upload_cloud(vox, np.zeros_like(vox), cam, scan["view_points"])
    ctx.estimate_normals(RADIUS)
    out = dict(M=len(vox), passes=0, nan=0, above=0, its=0, si=None)
    if s["k"] > 0:
        _, out["passes"], _, out["nan"] = ctx.refine_normals(s["k"])
    if s["sm"] is not None:
        sm = s["sm"] if s["ws"] is None else s["sm"][_inside(s["sm"], s["ws"])]
        hands, out["n_cand"] = ctx.detect_samples(sm)
        flat = hands.reshape(-1)
        out["records"] = flat[flat["valid"].astype(bool)].copy()
        out["S"] = len(sm)
        return out
    above = np.zeros(0, np.int32)
    if s["plane"]:
        above, _, _, out["its"] = ctx.sample_above_plane()
    out["above"] = len(above)
    if len(above):
        si = above[_with_repetition(len(above), s["draws"], s["seed"])]
    else:
        si = _dense_fisher_yates(len(vox), s["draws"], s["seed"])
    hands, _, out["n_cand"] = ctx.detect_select(si, 0)
    out["records"], out["si"], out["S"] = hands.copy(), si.astype(np.int32), len(si)
    return out


def build(ctx, specs):
    """One job array over specs that differ in workspace and route (Context.raw_batch takes one workspace per call)."""
    jobs = (api.DetectJob * len(specs))()
    keeps = []
    for i, s in enumerate(specs):
        one, keep = ctx.raw_batch([s["scan"]], [s["sm"]], s["ws"], CELL, RADIUS, refine_normals_k=s["k"], sample_above_plane=s["plane"],
                                  num_draws=s["draws"], sample_seed=s["seed"])
        jobs[i] = one[0]
        keeps.append(keep[0])
    return jobs, keeps


def run(ctx, jobs, expect_rc=0):
    rc = api.lib().gpd_hip_detect_batch(ctx._h, jobs, len(jobs))
    assert rc == expect_rc, (rc, api.lib().gpd_hip_last_error().decode())


def records(job, keep):
    return keep[5][: job.num_hands]


def check_job(j, keep, want, tag=""):
    print("%s status %d M %d/%d S %d/%d cand %d/%d above %d/%d its %d/%d passes %d/%d nan %d/%d preprocess_ms %s" % (
        tag, j.status, j.num_points_processed, want["M"], j.num_samples_processed, want["S"], j.num_candidates, want["n_cand"],
        j.plane_num_above, want["above"], j.plane_iterations, want["its"], j.refine_passes, want["passes"], j.refine_num_nan, want["nan"],
        [round(float(x), 2) for x in j.preprocess_ms]))
    assert j.status == 0, tag
    assert j.num_points_processed == want["M"] and j.num_samples_processed == want["S"], tag
    assert j.num_candidates == want["n_cand"] == j.num_hands, tag
    assert (j.refine_passes, j.refine_num_nan) == (want["passes"], want["nan"]), tag
    assert (j.plane_num_above, j.plane_iterations) == (want["above"], want["its"]), tag
    if want["si"] is not None:
        assert np.array_equal(keep[7][: j.num_samples_processed], want["si"]), tag
    assert records(j, keep).tobytes() == want["records"].tobytes(), tag


@pytest.fixture(scope="module")
def weights():
    return synth.lenet_weights(15, real=dict(np.load(os.path.join(GOLD, "lenet15_params.npz"))), trained_magnitude=True)


@pytest.fixture(scope="module")
def ctx(weights):
    c = api.Context(api.default_params(15))
    c.set_lenet_weights(weights)
    yield c
    c.close()


# seeds under which 150 draws from the above-plane list hit one entry twice (found on the host model of the fit; the test
# asserts the repeat on the stepwise side, so a seed that stops doing so fails the precondition instead of passing vacuously)
FULL_SEEDS = (11, 13, 12, 14)


@pytest.fixture(scope="module")
def full_specs():
    out = [spec(table_mug_scan(), None, None, 30, True, 150, FULL_SEEDS[0])]
    for i, n in enumerate((60000, 90000, 40000)):
        out.append(spec(synth_scan(700 + i, n)[0], WS, None, 30, True, 150, FULL_SEEDS[1 + i]))
    return out


@pytest.fixture(scope="module")
def full_want(ctx, full_specs):
    return [stepwise(ctx, s) for s in full_specs]


def test_full_flow_on_real_data(ctx, full_specs, full_want):
    """table_mug raw and three synthetic two-camera scans, ur5.cfg's flow — voxelise, normals, refineNormals(30),
    sampleAbovePlane, subsample(150) — in one batch of four, byte for byte against the stepwise route."""
    assert len(full_specs[0]["scan"]["xyz"]) == 104444
    for w in full_want:
        assert w["above"] > 150 and w["n_cand"] > 100 and w["passes"] > 0 and len(w["si"]) == 150
    assert any(len(set(w["si"].tolist())) < len(w["si"]) for w in full_want), "no job draws a sample index twice"
    jobs, keeps = build(ctx, full_specs)
    run(ctx, jobs)
    for i, (j, k, w, s) in enumerate(zip(jobs, keeps, full_want, full_specs)):
        check_job(j, k, w, "full %d" % i)
        assert j.num_samples_processed == 150 and j.num_sets <= 150 and j.lcg_draws > 0


def test_refinement_alone_on_the_coordinates_route(ctx):
    scan, sm = synth_scan(720, 60000)
    plain, refined = spec(scan, WS, sm), spec(scan, WS, sm, k=30, plane=True)  # the plane flag changes nothing on this route
    want_plain, want_refined = stepwise(ctx, plain), stepwise(ctx, refined)
    assert want_refined["passes"] > 0 and want_refined["n_cand"] > 100
    assert want_plain["records"].tobytes() != want_refined["records"].tobytes()
    jobs, keeps = build(ctx, [plain, refined])
    run(ctx, jobs)
    check_job(jobs[0], keeps[0], want_plain, "k = 0")
    check_job(jobs[1], keeps[1], want_refined, "k = 30")
    assert records(jobs[0], keeps[0]).tobytes() != records(jobs[1], keeps[1]).tobytes()
    assert jobs[1].plane_num_above == 0 and jobs[1].plane_iterations == 0  # the fit is not run at sample coordinates


def test_plane_alone_searches_the_whole_list_in_order(ctx):
    scan, _ = synth_scan(730, 30000)
    ws = np.array([-0.1, 0.1, -0.1, 0.1, -1.0, 1.0])  # a ninth of the table: the list stays in the low thousands
    probe = stepwise(ctx, spec(scan, ws, None, 0, True, 1, 0))
    assert 100 < probe["above"] < 5000
    s = spec(scan, ws, None, 0, True, probe["M"], 3)  # more draws than the list holds
    want = stepwise(ctx, s)
    assert len(want["si"]) == want["above"] == probe["above"] and np.all(np.diff(want["si"]) > 0) and want["n_cand"] > 100
    jobs, keeps = build(ctx, [s])
    run(ctx, jobs)
    check_job(jobs[0], keeps[0], want, "plane only")


def test_draws_alone_are_uniform_and_distinct(ctx):
    scan, _ = synth_scan(740, 60000)
    small, _ = synth_scan(741, 1500, base=1500)
    a = spec(scan, WS, None, 0, False, 150, 21)
    b = spec(small, None, None, 0, False, 10 ** 6, 22)  # more draws than points: every point once, shuffled
    wa, wb = stepwise(ctx, a), stepwise(ctx, b)
    assert len(set(wa["si"].tolist())) == 150 and wa["above"] == 0 and wa["n_cand"] > 100
    assert len(wb["si"]) == wb["M"] and sorted(wb["si"].tolist()) == list(range(wb["M"]))
    jobs, keeps = build(ctx, [a, b])
    run(ctx, jobs)
    check_job(jobs[0], keeps[0], wa, "uniform 150")
    check_job(jobs[1], keeps[1], wb, "uniform all")


def test_failed_fit_falls_back_to_the_whole_cloud(ctx):
    s = spec(flat_scan(), None, None, 0, True, 150, 31)
    want = stepwise(ctx, s)
    assert want["above"] == 0 and want["its"] > 0 and len(set(want["si"].tolist())) == 150
    # ... and a scan of which the cut leaves two points: no sample of three can be drawn, no hypothesis is evaluated
    two = two_point_scan()
    s2 = spec(two, TWO_WS, None, 0, True, 150, 32)
    want2 = stepwise(ctx, s2)
    assert want2["M"] == 2 and want2["above"] == 0 and want2["its"] == 0 and sorted(want2["si"].tolist()) == [0, 1]
    jobs, keeps = build(ctx, [s, s2])
    run(ctx, jobs)
    check_job(jobs[0], keeps[0], want, "flat table")
    assert jobs[0].plane_num_above == 0 and jobs[0].num_samples_processed == 150
    check_job(jobs[1], keeps[1], want2, "two points")
    assert jobs[1].plane_num_above == 0 and jobs[1].plane_iterations == 0 and jobs[1].num_samples_processed == 2


def test_zero_fields_change_nothing(ctx):
    scan, sm = synth_scan(750, 60000)
    old, keep_old = ctx.raw_batch([scan], [sm], WS, CELL, RADIUS)
    new, keep_new = ctx.raw_batch([scan], [sm], WS, CELL, RADIUS, refine_normals_k=0, sample_above_plane=False, num_draws=0, sample_seed=0)
    for name, _ in api.DetectJob._fields_:
        if name in ("refine_normals_k", "sample_above_plane", "num_draws", "sample_seed", "samples_out", "refine_passes", "refine_num_nan",
                    "plane_num_above", "plane_iterations"):
            assert not getattr(old[0], name) and not getattr(new[0], name), name
    sentinel = np.full(64, -77, np.int32)
    new[0].samples_out = api._ptr(sentinel)
    run(ctx, old)
    run(ctx, new)
    assert old[0].num_hands == new[0].num_hands > 100
    assert records(old[0], keep_old[0]).tobytes() == records(new[0], keep_new[0]).tobytes()
    assert old[0].num_samples_processed == new[0].num_samples_processed and old[0].lcg_draws == new[0].lcg_draws > 0
    assert np.all(sentinel == -77)
    want = stepwise(ctx, spec(scan, WS, sm))
    check_job(old[0], keep_old[0], want, "old keywords")


def test_mixed_batch_on_both_lanes(ctx, full_specs, full_want):
    """Full-flow jobs and plain coordinate jobs alternate, so both lanes run fits and refinements of different sizes next to
    each other's searches: one plane / refinement state shared across the two streams shows here."""
    specs, want = [], []
    coords = [synth_scan(760 + i, n) for i, n in enumerate((75000, 40000, 90000, 60000))]
    for i in range(4):
        specs.append(full_specs[(i + 1) % 4])
        want.append(full_want[(i + 1) % 4])
        specs.append(spec(coords[i][0], WS if i != 2 else None, coords[i][1]))
        want.append(stepwise(ctx, specs[-1]))
    # lane 0 takes jobs 0, 2, 4, 6, lane 1 the odd ones: swap one pair so each lane sees both kinds
    specs[2], specs[3] = specs[3], specs[2]
    want[2], want[3] = want[3], want[2]
    jobs, keeps = build(ctx, specs)
    run(ctx, jobs)
    for i, (j, k, w, s) in enumerate(zip(jobs, keeps, want, specs)):
        check_job(j, k, w, "mixed %d" % i)
    first = [(records(j, k).tobytes(), bytes(k[7][: j.num_samples_processed]) if k[7] is not None else b"") for j, k in zip(jobs, keeps)]
    run(ctx, jobs)
    for i, (j, k) in enumerate(zip(jobs, keeps)):
        again = (records(j, k).tobytes(), bytes(k[7][: j.num_samples_processed]) if k[7] is not None else b"")
        assert again == first[i], i


def test_errors_stay_per_job(ctx, full_specs, full_want):
    scan, sm = synth_scan(770, 40000)
    good_coords = spec(scan, WS, sm)
    want_coords = stepwise(ctx, good_coords)
    bad_both = spec(scan, WS, sm, draws=10)
    specs = [full_specs[1], spec(scan, WS, sm, k=257), good_coords, spec(scan, WS, sm, k=-1), bad_both,
             spec(scan, WS, None, draws=-5), full_specs[3]]
    jobs, keeps = build(ctx, specs)
    run(ctx, jobs, expect_rc=-3)  # the first error of the batch: GPD_ERR_CAPACITY of job 1
    assert "257" in api.lib().gpd_hip_last_error().decode()
    assert [j.status for j in jobs] == [0, -3, 0, -1, -1, -1, 0]
    for i in (1, 3, 4, 5):
        assert jobs[i].num_hands == 0 and jobs[i].num_candidates == 0
    check_job(jobs[0], keeps[0], full_want[1], "before the errors")
    check_job(jobs[2], keeps[2], want_coords, "between the errors")
    check_job(jobs[6], keeps[6], full_want[3], "after the errors")


def test_batch_multi_over_two_contexts(ctx, weights, full_specs, full_want):
    other = api.Context(api.default_params(15))
    try:
        other.set_lenet_weights(weights)
        specs = full_specs + [full_specs[2]]
        want = full_want + [full_want[2]]
        jobs, keeps = build(ctx, specs)
        arr = (C.c_void_p * 2)(ctx._h, other._h)
        rc = api.lib().gpd_hip_detect_batch_multi(arr, 2, jobs, len(jobs))
        assert rc == 0, api.lib().gpd_hip_last_error().decode()
        for i, (j, k, w, s) in enumerate(zip(jobs, keeps, want, specs)):
            check_job(j, k, w, "multi %d" % i)
    finally:
        other.close()


def test_a_raw_job_images_with_the_shadow_jitter_of_its_context(weights):
    """gpd_hip_set_shadow_jitter holds for a raw job of gpd_hip_detect_batch as for the single calls: with the setting on the
    job returns the records of preprocess_cloud + upload_cloud + detect_samples on the same context byte for byte, and their
    scores are not those of the setting off; off again, the job returns the first records again."""
    scan, sm = synth_scan(780, 16000, base=8000)
    s = spec(scan, WS, sm[:24])
    c = api.Context(api.default_params(15))
    try:
        c.set_lenet_weights(weights)
        off = stepwise(c, s)
        c.set_shadow_jitter(True, 0x5EED5EED5EED)
        on = stepwise(c, s)
        assert on["n_cand"] == off["n_cand"] >= 20 and on["M"] == off["M"]
        a, b = on["records"].copy(), off["records"].copy()
        differ = int((a["score"] != b["score"]).sum())
        print("raw job: %d of %d scores differ with the jitter on" % (differ, len(a)))
        assert differ >= 1
        a["score"] = b["score"] = 0
        assert a.tobytes() == b.tobytes()
        jobs, keeps = build(c, [s])
        run(c, jobs)
        check_job(jobs[0], keeps[0], on, "jitter on")
        assert records(jobs[0], keeps[0])["score"].tobytes() != off["records"]["score"].tobytes()
        c.set_shadow_jitter(False)
        run(c, jobs)
        check_job(jobs[0], keeps[0], off, "jitter off again")
    finally:
        c.close()
