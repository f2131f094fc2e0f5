"""cem_detect_grasps with cfg hip_sis_resident = 1: SequentialImportanceSampling::detectGrasps as ONE gpd_hip_detect_sis call.  The
samples it used are dumped (GPD_SIS_DUMP, the same file format as the host loop writes) and replayed through the oracle, as
tests/test_host_cli.py::test_cem_detect_grasps_matches_oracle_replay does for the key's default."""
import os
import subprocess

import numpy as np
import pytest

import pyref_sample
import pyref_sis
import sis_cases as sc
from gpd_amd import synth
from test_host_cli import CEM, _subsample_indices, _write_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("method,min_inliers", [(0, 0), (1, 0), (0, 1)])
def test_cem_detect_grasps_resident_matches_oracle_replay(tmp_path, oracle_mod, lenet15_real, method, min_inliers):
    assert os.path.exists(CEM), "run __graft_entry__.build()"
    cl = synth.make_cloud(99, 12000)
    cfg, pcd = _write_case(tmp_path, cl, lenet15_real, 100, 50, min_inliers=min_inliers,
                           extra="num_init_samples = 40\nnum_iterations = 3\nnum_samples_per_iteration = 40\nprob_rand_samples = 0.3\n"
                                 "standard_deviation = 0.02\nsampling_method = %d\nmin_score = -300\nrandom_seed = 7\n"
                                 "hip_sis_resident = 1\n" % method)
    dump = tmp_path / "sis_samples.txt"
    env = dict(os.environ, GPD_SIS_DUMP=str(dump))
    out = subprocess.run([CEM, str(cfg), str(pcd)], capture_output=True, text=True, cwd=str(tmp_path), timeout=300, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = [l.split() for l in out.stdout.splitlines() if l.startswith("GRASP ")]
    # ---- the dump
    lines = dump.read_text().splitlines()
    n_init = int(lines[0].split()[1])
    idx = np.array([int(x) for x in lines[1:1 + n_init]], np.int32)
    rounds, k = [], 1 + n_init
    while k < len(lines):
        assert lines[k].split()[:2] == ["ROUND", str(len(rounds))]
        n = int(lines[k].split()[2])
        rounds.append(np.array([[float(v) for v in l.split()] for l in lines[k + 1:k + 1 + n]], np.float64))
        k += 1 + n
    assert len(rounds) == 3 and all(len(r) == 40 for r in rounds)
    # cloud.subsample(num_init_samples) on the 100 sample indices the preprocessing left: 40 draws with repetition
    assert np.array_equal(idx, _subsample_indices(len(cl["xyz"]), 100)[pyref_sample.with_repetition(100, 40, 0)])
    assert all(np.isin(r[28:].astype(np.float32), cl["xyz"][idx]).all() for r in rounds)  # 12 cloud points per round
    # ---- replay through the oracle
    p = oracle_mod.default_params(15)
    want = sc.replay(oracle_mod, p, cl, cl["cam_source"], cl["view_points"], idx, rounds, lenet15_real, -300.0, min_inliers)
    assert all(n >= 1 for n in want["live"]) and len(want["hands"]) > 5
    # the lines of the rounds come from round_counts
    total = want["live"][0]
    assert ("Grasps within workspace: %d" % total) in out.stdout
    for r in range(3):
        total += want["live"][r + 1]
        assert ("Added %d grasp candidates in round %d. Total: %d." % (want["live"][r + 1], r, total)) in out.stdout
    # ---- the draws are the seeded streams: random_seed is the seed
    pred = sc.predict(oracle_mod, p, cl, cl["cam_source"], cl["view_points"], idx, lenet15_real, 7, method, min_inliers=min_inliers)
    assert np.array(rounds).tobytes() == pred["samples"].tobytes()
    # ---- the printed grasps, within the allowances of the test of the key's default
    wh = want["hands"]
    assert len(got) == len(wh)
    gs = np.array([float(g[1]) for g in got])
    assert np.abs(gs - wh["score"].astype(np.float64)).max() <= 2e-4
    gp = np.array([[float(x) for x in g[2:5]] for g in got])
    assert np.allclose(gp, wh["position"], rtol=1e-9, atol=1e-12)
    assert [int(g[6]) for g in got] == wh["finger_placement_index"].tolist()
    assert pyref_sis.num_rand_samples(0.3, 40) == 12
