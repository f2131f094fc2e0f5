"""The host mirror with hand sets that are not the last search's (tests/host/given_hands_selftest.cpp): the hand sets one
gpd::GraspDetector finds on one cloud, imaged (createImages) and pruned (pruneGraspCandidates) by another detector over a
modified cloud, must equal the Python route — Context.images_given / score_given of the same records on that cloud."""
import os
import subprocess

import numpy as np
import pytest

import given_cases as gc
from gpd_amd import api, synth
from test_host_cli import _write_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_pcd(path, xyz, normals):
    P = len(xyz)
    with open(str(path), "w") as f:
        f.write("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z normal_x normal_y normal_z\n"
                "SIZE 4 4 4 4 4 4\nTYPE F F F F F F\nCOUNT 1 1 1 1 1 1\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA ascii\n" % (P, P))
        for p, n in zip(xyz, normals):
            f.write("%.9g %.9g %.9g %.9g %.9g %.9g\n" % (p[0], p[1], p[2], n[0], n[1], n[2]))


def test_driver_equals_the_python_route(tmp_path, lenet15_real):
    exe = os.path.join(ROOT, "gpd_amd", "host", "given_hands_selftest")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    cl, _ = gc.scene(two_cameras=False)
    cfg, pcd = _write_case(tmp_path, cl, lenet15_real, 60, 4000)
    keep = np.arange(len(cl["xyz"])) % 10 != 0
    other_xyz = np.ascontiguousarray(synth.off_lattice(cl)["xyz"][keep])
    other_nrm = np.ascontiguousarray(cl["normals"][keep])
    pcd2 = tmp_path / "other.pcd"
    _write_pcd(pcd2, other_xyz, other_nrm)
    prefix = tmp_path / "dump"
    out = subprocess.run([exe, str(cfg), str(pcd), str(pcd2), str(prefix)], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("SELFTEST OK"), out.stdout[-1500:] + out.stderr[-1000:]
    assert "ERROR" not in out.stdout
    given = np.fromfile(str(prefix) + ".given", api.HAND_DTYPE).reshape(-1, 8)
    hands = np.fromfile(str(prefix) + ".hands", api.HAND_DTYPE)
    pruned = np.fromfile(str(prefix) + ".pruned", api.HAND_DTYPE)
    n = len(hands)
    images = np.fromfile(str(prefix) + ".images", np.uint8).reshape(n, 60, 60, 15)
    assert 20 <= len(given) <= 60 and n == int(given["valid"].sum()) > 50 and len(pruned) == n
    # the Python route on the same records and the same cloud (the PCD's nine digits carry every float32 exactly)
    ctx = api.Context(api.default_params(15))
    try:
        ctx.set_lenet_weights(lenet15_real)
        ctx.upload_cloud(other_xyz, other_nrm)
        gimg, cand, _ = ctx.images_given(given)
        scored, scores, cand2, _ = ctx.score_given(given)
    finally:
        ctx.close()
    assert np.array_equal(cand, cand2)
    assert images.tobytes() == gimg.tobytes()
    assert hands.tobytes() == given.ravel()[cand].tobytes()
    assert pruned.tobytes() == scored.ravel()[cand].tobytes()
    assert pruned["score"].tobytes() == scores.tobytes() and len(np.unique(scores)) > n // 2
