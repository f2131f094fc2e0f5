"""What every composed entry of the library must return on a variant of tests/ref_cases.py, composed from the oracle alone and
computed once per variant: detect / detect_select, detect_samples, the batch entries (three jobs), images_given / score_given,
detect_sis and label_view.  tests/test_entry_cases.py proves on the CPU that none of these expectations is empty;
tests/test_gpu_entries_by_variant.py runs the library against them.  Inside `with jitter(om, seed):` the same functions give
the expectations of gpd_hip_set_shadow_jitter(on, seed), from the oracle's own statement of that policy
(tests/test_gpu_entries_by_variant_jitter.py).  Nothing here is modified after it is built."""
import numpy as np

import label_view_cases as lvc
import ref_cases as rcs
import sis_cases as sc
from gpd_amd import synth

SELECT_K = 7
NUDGE_SEED, NUDGE = 5, 0.003                 # detect_samples: the sample points moved by up to 3 mm per axis
JOB1_SAMPLES, JOB1_CLOUD_SEED = 20, 11       # the batch's second job: another cloud, another draw of samples, one camera
LCG_BASES = (0, 12345678901)
SIS = dict(seed=7, method=0, rounds=2, per=24, min_score=-300.0, min_inliers=0)
GT_SEED, ROUNDS_SEED, VIEW_ROUNDS, SAMPLES_PER_ROUND = 7, 7, 4, 16
MIN_POSITIVES, MAX_GRASPS_PER_VIEW = 10 ** 6, 500  # no round stops the view early
# the shadow jitter (gpd_hip_set_shadow_jitter): the seed, and the variants every entry also runs on with the setting on — the
# window-class transitions of image::window_class (stock 0 -> 1, one voxel to spare, 1 -> 1, wide -> general, general -> general),
# a channel count without a shadow, 24 slots, a 12-way set intersection with a blind camera, off-lattice input with two cameras
JITTER_SEED = 0x5EED5EED5EED
JITTER_VARIANTS = ("default_c15", "default_c12", "other_image_volume", "wide_image_volume", "huge_image_volume", "deep_hand",
                   "three_axes", "twelve_cameras", "offlattice_two_cameras")

_cache = {}


def _once(om, kind, name, make):
    """One expectation per (kind, variant, shadow-jitter seed of the oracle or None): what was composed with the setting off is
    never returned with it on, nor the reverse.  The seed is read back from the oracle itself (entry_cases.jitter below)."""
    key = (kind, name, om.shadow_jitter_state())
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _freeze(v)
    return x


def jitter(om, seed):
    """with jitter(om, seed): every expectation built or fetched inside is the one of gpd_hip_set_shadow_jitter(on, seed); seed
    None: off, as outside.  The oracle is switched off again on the way out."""
    return om.shadow_jitter(seed)


def slots(p):
    return p.num_hand_axes * p.num_orientations


def inputs(name, default_params):
    """(params, cloud dict carrying the variant's cameras, sample indices, weights) for whoever runs the case."""
    p, cl, si, cam, vp = rcs.case_inputs(name, default_params)
    cl = dict(cl, cam_source=np.ascontiguousarray(cam, np.int32).reshape(-1, len(cl["xyz"])),
              view_points=np.ascontiguousarray(vp, np.float64).reshape(-1, 3))
    return p, cl, si, rcs.weights(p.image_num_channels, trained_magnitude=True)


def _detect(om, p, cl, si, w):
    """oracle.detect -> dict(hands [sets, slots], cands: the valid records in (set, slot) order, n_sets, n_cand, top: the
    indices selectGrasps(SELECT_K) keeps)."""
    if not len(si):
        z = np.zeros(0, om.HAND_DTYPE)
        return dict(hands=z.reshape(0, slots(p)), cands=z, n_sets=0, n_cand=0, top=np.zeros(0, np.int32))
    hands, n_cand, _ = om.detect(p, cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"], si, w)
    flat = hands.reshape(-1)
    cands = flat[flat["valid"].astype(bool)].copy()
    assert len(cands) == n_cand
    top = om.select(cands["score"], SELECT_K) if n_cand else np.zeros(0, np.int32)
    return dict(hands=hands, cands=cands, n_sets=len(hands), n_cand=n_cand, top=top)


def selected(want, k):
    """The records detect_select / a batch job returns for num_selected = k (0: every candidate; otherwise SELECT_K)."""
    assert k in (0, SELECT_K)
    return want["cands"] if k == 0 else want["cands"][want["top"]]


def detect(om, name):
    def make():
        p, cl, si, w = inputs(name, om.default_params)
        return _freeze(_detect(om, p, cl, si, w))
    return _once(om, "detect", name, make)


def sample_points(name):
    """detect_samples' coordinates: the variant's sample points, each moved by a seeded nudge."""
    cl = rcs.cloud(name)
    si = synth.sample_indices(cl, rcs.NUM_SAMPLES)  # rcs.case_inputs' draw
    rng = np.random.RandomState(NUDGE_SEED)
    return cl["xyz"][si].astype(np.float64) + rng.uniform(-NUDGE, NUDGE, (len(si), 3))


def _score_sets(om, p, cl, sets, w):
    """filter_workspace -> images -> lenet over hand sets [n, slots] -> (the sets with flags filtered and scores written,
    images, cand_index, scores)."""
    hands = om.filter_workspace(p, sets.copy()) if len(sets) else sets.copy()
    img, cand = om.images(p, cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"], hands)
    scores = om.lenet(img, w) if len(cand) else np.zeros(0, np.float32)
    flat = hands.reshape(-1)
    flat["score"][cand] = scores
    return hands, img, cand, scores


def detect_samples(om, name):
    def make():
        p, cl, si, w = inputs(name, om.default_params)
        sets = om.search_xyz(p, cl["xyz"], cl["normals"], sample_points(name))
        hands, img, cand, scores = _score_sets(om, p, cl, sets, w)
        return _freeze(dict(hands=hands, n_cand=len(cand), cand=cand, scores=scores))
    return _once(om, "detect_samples", name, make)


def batch_jobs(name, default_params):
    """(clouds, samples) of the three jobs: the variant's cloud with its cameras; the cloud moved off its coordinates with ONE
    camera and another draw of 20 samples; the variant's cloud without samples."""
    _, cl, si, _ = inputs(name, default_params)
    base = rcs.cloud(name)
    other = synth.off_lattice(base, seed=JOB1_CLOUD_SEED)  # keeps the one camera and the view point of the synthetic cloud
    assert other["cam_source"].shape[0] == 1 and cl["cam_source"].shape[0] == rcs.VARIANTS[name][2]
    s1 = synth.sample_indices(base, JOB1_SAMPLES, seed=rcs.CLOUD_SEED + 1)
    return [cl, other, cl], [si, s1, si[:0]]


def batch(om, name):
    """Per job what detect() returns for it."""
    def make():
        p, _, _, w = inputs(name, om.default_params)
        clouds, samples = batch_jobs(name, om.default_params)
        out = [detect(om, name)] + [_detect(om, p, cl, s, w) for cl, s in zip(clouds[1:], samples[1:])]
        return _freeze(out)
    return _once(om, "batch", name, make)


def given_sets(om, name):
    """The hand sets handed to images_given / score_given: (a) the oracle's searched and workspace-filtered records [24, slots];
    (b) the same with the set order reversed and every third valid flag (in the new order) cleared."""
    def make():
        p, cl, si, _ = inputs(name, om.default_params)
        a = om.filter_workspace(p, om.search(p, cl["xyz"], cl["normals"], si))
        b = np.ascontiguousarray(a[::-1]).copy()
        flat = b.reshape(-1)
        flat["valid"][np.flatnonzero(flat["valid"])[::3]] = 0
        return _freeze(dict(a=a, b=b))
    return _once(om, "given_sets", name, make)


def given(om, name, which, lcg_base):
    """dict(images, cand, draws, scores) of given_sets()[which] with the shadow stream starting at lcg_base."""
    def make():
        p, cl, _, w = inputs(name, om.default_params)
        om.set_lcg_base(lcg_base)
        try:
            img, cand = om.images(p, cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"], given_sets(om, name)[which])
            draws = om.last_lcg_draws()
        finally:
            om.set_lcg_base(0)
        return _freeze(dict(images=img, cand=cand, draws=draws, scores=om.lenet(img, w) if len(cand) else np.zeros(0, np.float32)))
    return _once(om, "given_%s_%d" % (which, lcg_base), name, make)


def shard_draws(om, name, cut):
    """Shadow draws of the hand sets of the samples before `cut` and of those from it on: what detect_sharded's two ranges
    consume of the cloud's one stream."""
    def make():
        p, cl, _, _ = inputs(name, om.default_params)
        a = given_sets(om, name)["a"]
        assert len(a) == rcs.NUM_SAMPLES  # every sample has its hand set: sets and samples are numbered alike
        om.images(p, cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"], a[:cut], want_images=False)
        head = om.last_lcg_draws()
        return head, given(om, name, "a", 0)["draws"] - head
    return _once(om, "shard_draws_%d" % cut, name, make)


def nonempty(images):
    return int((images.reshape(len(images), -1).max(axis=1) > 0).sum()) if len(images) else 0


def sis_predict(om, name):
    def make():
        p, cl, si, w = inputs(name, om.default_params)
        return _freeze(sc.predict(om, p, cl, cl["cam_source"], cl["view_points"], si, w, **SIS))
    return _once(om, "sis", name, make)


def sis_replay(om, name, samples):
    """sis_cases.replay on the samples a run returned (not cached: they are the device's)."""
    p, cl, si, w = inputs(name, om.default_params)
    return sc.replay(om, p, cl, cl["cam_source"], cl["view_points"], si, samples, w, SIS["min_score"], SIS["min_inliers"])


def view_rounds(name):
    """4 rounds of 16 sample indices, drawn as tests/test_gpu_label_view.py draws its rounds."""
    cl = rcs.cloud(name)
    rng = np.random.RandomState(ROUNDS_SEED)
    obj = np.flatnonzero(cl["is_object"])
    return np.stack([rng.choice(obj, SAMPLES_PER_ROUND, replace=False) for _ in range(VIEW_ROUNDS)]).astype(np.int32)


def ground_truth(name):
    cl = rcs.cloud(name)
    gt, gn, _ = rcs.ground_truth(cl["xyz"], cl["normals"], GT_SEED)
    return gt, gn


def view(om, name):
    def make():
        p, cl, _, _ = inputs(name, om.default_params)
        gt, gn = ground_truth(name)
        return _freeze(lvc.expected_view(om, p, cl["xyz"], cl["normals"], cl["cam_source"], cl["view_points"], gt, gn, view_rounds(name),
                                         MIN_POSITIVES, MAX_GRASPS_PER_VIEW))
    return _once(om, "view", name, make)
