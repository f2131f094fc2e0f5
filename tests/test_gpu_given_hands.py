"""gpd_hip_images_given / gpd_hip_score_given: images and scores of hand sets the caller supplies, not only the last search's
(ImageGenerator::createImages(cloud, hand_set_list), image_generator.cpp:17-99).  The oracle's gpd_oracle_images takes arbitrary
records and is the definition; every comparison is byte for byte."""
import numpy as np
import pytest

import given_cases as gc
from gpd_amd import api, synth

pytestmark = pytest.mark.gpu

LCG_BASE = 12345678901


def _upload(ctx, cl):
    ctx.upload_cloud(cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"])


def _oracle_images(oracle, C, cl, hands, lcg_base=0):
    op = oracle.default_params(C)
    oracle.set_lcg_base(lcg_base)
    try:
        img, cand = oracle.images(op, cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"], hands)
        return img, cand, oracle.last_lcg_draws()
    finally:
        oracle.set_lcg_base(0)


def _nonempty(img):
    return int((img.reshape(len(img), -1).max(axis=1) > 0).sum()) if len(img) else 0


@pytest.fixture(scope="module")
def searched():
    """The scene (two cameras) and, per channel count, the records ctx.search returns for its 48 samples with the images
    ctx.images makes of them; computed once, never modified."""
    cl, si = gc.scene()
    out = {}
    for C in (1, 3, 12, 15):
        ctx = api.Context(api.default_params(C))
        try:
            _upload(ctx, cl)
            hands = ctx.search(si)
            img, cand = ctx.images(hands)
        finally:
            ctx.close()
        for a in (hands, img, cand):
            a.setflags(write=False)
        out[C] = (hands, img, cand)
    return cl, si, out


@pytest.mark.parametrize("C", [1, 3, 12, 15])
def test_round_trip_of_the_search_records(oracle_mod, searched, C):
    cl, si, per = searched
    hands, img, cand = per[C]
    p = api.default_params(C)
    assert hands.shape == (gc.NUM_SAMPLES, 8) and len(cand) > 50
    assert api.given_check(p, hands) is None  # the check's slack admits every record of the project's own search
    ctx = api.Context(p)
    try:
        _upload(ctx, cl)
        gimg, gcand, draws = ctx.images_given(hands)
    finally:
        ctx.close()
    assert np.array_equal(gcand, cand)
    assert gimg.tobytes() == img.tobytes()
    assert _nonempty(gimg) >= 0.9 * len(gimg)
    want_draws = _oracle_images(oracle_mod, C, cl, hands)[2]
    print("round trip C=%d: %d candidates, %d shadow draws" % (C, len(cand), draws))
    assert draws == want_draws and (draws > 0) == (C == 15)


@pytest.mark.parametrize("C", [3, 15])
def test_foreign_hands_equal_the_oracle(oracle_mod, searched, C):
    cl, si, per = searched
    f, off, far = gc.foreign(per[C][0], cl["normals"][si])
    p = api.default_params(C)
    assert api.given_check(p, f) is None
    # the construction holds what it promises: sets without a frame neighbourhood, sets without an image neighbourhood, with valid hands
    for s in off:
        assert len(oracle_mod.radius_search(cl["xyz"], f[s, 0]["sample"], p.nn_radius_frames)[0]) == 0
    for s in far:
        assert len(oracle_mod.radius_search(cl["xyz"], f[s, 0]["sample"], 0.10)[0]) == 0
    assert int(f["valid"][off].sum()) > 0 and int(f["valid"][far].sum()) > 0
    assert not f["valid"][[len(f) - 1 - s for s in range(0, len(f), 5)]].any()
    ctx = api.Context(p)
    try:
        _upload(ctx, cl)
        for base in (0, LCG_BASE):
            wimg, wcand, wdraws = _oracle_images(oracle_mod, C, cl, f, base)
            n, ne = len(wcand), _nonempty(wimg)
            print("foreign C=%d lcg_base=%d: %d candidates, %d non-empty images, %d draws" % (C, base, n, ne, wdraws))
            assert n >= 100 and ne >= 0.75 * n  # the comparison cannot pass on empty images
            gimg, gcand, gdraws = ctx.images_given(f, lcg_base=base)
            assert np.array_equal(gcand, wcand)
            assert gdraws == wdraws
            bad = np.flatnonzero((gimg != wimg).reshape(n, -1).any(axis=1))
            assert gimg.tobytes() == wimg.tobytes(), (len(bad), bad[:10], gcand[bad[:10]] // 8)
        if C == 15:  # the stream position matters: another base, other shadow channels
            assert _oracle_images(oracle_mod, C, cl, f, 0)[0].tobytes() != wimg.tobytes()
    finally:
        ctx.close()


@pytest.mark.parametrize("C", [3, 15])
def test_hands_of_one_cloud_on_another(oracle_mod, searched, C):
    cl, si, per = searched
    hands = per[C][0]
    keep = np.arange(len(cl["xyz"])) % 10 != 0
    moved = synth.off_lattice(cl)
    other = dict(xyz=np.ascontiguousarray(moved["xyz"][keep]), normals=np.ascontiguousarray(cl["normals"][keep]),
                 cam_source=np.ascontiguousarray(cl["cam_source"][:, keep]), view_points=cl["view_points"])
    wimg, wcand, wdraws = _oracle_images(oracle_mod, C, other, hands)
    assert wimg.tobytes() != per[C][1].tobytes()  # the other cloud gives other images
    ctx = api.Context(api.default_params(C))
    try:
        _upload(ctx, other)
        gimg, gcand, gdraws = ctx.images_given(hands)
    finally:
        ctx.close()
    assert np.array_equal(gcand, wcand) and gdraws == wdraws
    assert gimg.tobytes() == wimg.tobytes()
    assert _nonempty(gimg) >= 0.9 * len(gimg)


@pytest.mark.parametrize("mode", [api.LENET_SPLIT, api.LENET_F32_CHAIN])
def test_scores(oracle_mod, searched, lenet15_real, mode):
    cl, si, per = searched
    f, _, _ = gc.foreign(per[15][0], cl["normals"][si])
    f["score"] = 7.25  # what the call must overwrite on the valid records and leave on the others
    before = f.copy()
    ctx = api.Context(api.default_params(15))
    try:
        ctx.set_lenet_weights(lenet15_real)
        ctx.set_lenet_mode(mode)
        _upload(ctx, cl)
        out, scores, cand, draws = ctx.score_given(f)
        assert f.tobytes() == before.tobytes()  # the binding scores a copy
        n = len(cand)
        _, cand2, draws2 = ctx.images_given(f, download=False)
        again = ctx.score(None, n)
    finally:
        ctx.close()
    assert n >= 100 and np.array_equal(cand, cand2) and draws == draws2
    assert scores.tobytes() == again.tobytes()
    assert np.all(np.isfinite(scores)) and len(np.unique(scores)) > n // 2
    if mode == api.LENET_F32_CHAIN:
        wimg, wcand, _ = _oracle_images(oracle_mod, 15, cl, f)
        assert np.array_equal(wcand, cand)
        assert scores.tobytes() == oracle_mod.lenet(wimg, lenet15_real).tobytes()
    # `score` lands on the valid records; no other byte of the records changes
    valid = before["valid"].astype(bool)
    assert np.array_equal(np.flatnonzero(valid.ravel()), cand)
    assert out["score"].ravel()[cand].tobytes() == scores.tobytes()
    assert np.all(out["score"][~valid] == np.float32(7.25))
    rest = out.copy()
    rest["score"] = before["score"]
    assert rest.tobytes() == before.tobytes()


def test_large_lists_and_full_boxes(oracle_mod):
    """The large routes at their smallest: three lattice planes 3 mm apart put some 12 000 points within the list radius of the
    centre (past the 8192-entry lists: the 16384-entry ones), and boxes that lie in the planes hold some 2400 of them (past
    PT_CAP = 1024: the large points instantiation)."""
    k = np.arange(-40, 41)
    gx, gy, gz = np.meshgrid(k, k, np.arange(-1, 2), indexing="ij")
    key = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], 1).astype(np.float64)
    rng = np.random.RandomState(2)
    key = key[rng.permutation(len(key))]
    xyz = (key * 0.003 + np.array([0.0, 0.0, -0.501])).astype(np.float32)
    P = len(xyz)
    nrm = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (P, 1))
    cam = np.ones((2, P), np.int32)
    cam[1] = rng.rand(P) < 0.5
    cl = dict(xyz=xyz, normals=nrm, cam_source=cam, view_points=gc.VIEW_POINTS_2)
    p = api.default_params(15)
    hands = np.zeros((2, 8), api.HAND_DTYPE)
    c, s = np.cos(0.3), np.sin(0.3)
    frames = [np.eye(3), np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])]  # the hand axis along the planes' normal
    for si_, (smp, F) in enumerate(zip(([0.0, 0.0, -0.501], [0.0015, -0.0015, -0.5]), frames)):
        hands["sample"][si_] = smp
        hands["frame"][si_] = F.ravel()
    hands["valid"][0, [1, 6]] = 1
    hands["valid"][1, [0, 3, 7]] = 1
    hands["bottom"][:] = rng.uniform(-0.05, 0.0, (2, 8))
    hands["center"][:] = rng.uniform(-0.055, 0.055, (2, 8))
    assert api.given_check(p, hands) is None
    assert len(oracle_mod.radius_search(xyz, hands["sample"][0, 0], 0.10)[0]) > 8192
    wimg, wcand, wdraws = _oracle_images(oracle_mod, 15, cl, hands)
    ctx = api.Context(p)
    try:
        _upload(ctx, cl)
        gimg, gcand, gdraws = ctx.images_given(hands)
        fb = ctx.fallbacks()
    finally:
        ctx.close()
    print("large routes:", fb, "draws", gdraws)
    assert np.array_equal(gcand, wcand) and len(gcand) == 5 and gdraws == wdraws > 0
    assert gimg.tobytes() == wimg.tobytes() and _nonempty(gimg) == 5
    assert fb["neighbourhood_list_capacity"] == 16384
    assert fb["large_points_kernel_candidates"] == 5


def test_refusals_and_state(searched, lenet15_real):
    cl, si, per = searched
    hands = per[15][0]
    p = api.default_params(15)
    ctx = api.Context(p)
    try:
        ctx.set_lenet_weights(lenet15_real)
        with pytest.raises(api.GpdHipError, match=r"error -4: .*no cloud"):  # GPD_ERR_STATE
            ctx.images_given(hands)
        with pytest.raises(api.GpdHipError, match=r"error -4: .*no cloud"):
            ctx.score_given(hands)
        _upload(ctx, cl)
        det0, n0 = ctx.detect(si)
        det0 = det0.copy()
        mine = ctx.search(si)
        assert mine.tobytes() == hands.tobytes()
        for name, h, s, j in gc.refusals(hands, p):
            for call in (ctx.images_given, ctx.score_given):
                with pytest.raises(api.GpdHipError, match=r"error -1: .*set %d, slot %d" % (s, j)):  # GPD_ERR_INVALID
                    call(h)
        # nothing was enqueued and no state touched: the last search's records are still imaged, the same detect comes back
        img, cand = ctx.images(mine)
        assert img.tobytes() == per[15][1].tobytes() and np.array_equal(cand, per[15][2])
        det1, n1 = ctx.detect(si)
        assert n1 == n0 and det1.tobytes() == det0.tobytes()
        # the search buffers are reused: records of an earlier search are refused afterwards, as after reevaluate
        mine = ctx.search(si)
        ctx.images_given(mine[:5])
        with pytest.raises(api.GpdHipError, match=r"error -4: images: hands must come from"):
            ctx.images(mine)
        # ... and the context goes on: a new search, its images
        mine = ctx.search(si)
        img, cand = ctx.images(mine)
        assert img.tobytes() == per[15][1].tobytes()
        # no sets at all: no candidates
        img, cand, draws = ctx.images_given(mine[:0])
        assert len(cand) == 0 and draws == 0
    finally:
        ctx.close()
    bare = api.Context(p)
    try:
        _upload(bare, cl)
        with pytest.raises(api.GpdHipError, match=r"error -4: .*weights"):
            bare.score_given(hands)
        assert bare.images_given(hands)[0].tobytes() == per[15][1].tobytes()
    finally:
        bare.close()
