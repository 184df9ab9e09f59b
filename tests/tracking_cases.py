"""TEST INFRASTRUCTURE, not a test.  The cases and the rules of the tests that pin the kernels behind the matcher, feature
alignment, pose optimizer, point optimizer and depth filter (rows a8-a13 of DESIGN.md) to the reference -- once, for the host
emulation (tests/tracking_emulated.py runs them) and for the device (tests/tracking_device.py).  Plain numpy, oracle.pytrack,
rpg_svo_amd.synth / se3 and helpers: nothing here touches a GPU or loads the library under test.

  * Case: a scene with its inputs as columns (observations, features, seeds, epipolar queries) and the checker's answers,
    computed once per (case, checker, options) and shared by every test of a session.  committed(kind) is the scene of
    tests/test_tracking_gpu.py, test_track_emulated.py and test_optimizers_emulated.py; tests/track_edge_cases.py builds the
    same class from its own scenes.
  * verify_* / check_*: the comparison rules.  Tolerances: the float pipelines (feature alignment, affine warp) and every
    integer result (patch bytes, ZMSSD argmin, statuses, pruning flags) are IDENTICAL to the checker's -- the kernels keep the
    reference's evaluation order and run with contraction off; f64 geometry may differ in the last bits (libm sin / cos /
    acos / atan, quaternion selects), so poses, depths and covariances carry the tolerance stated at their assert.
    tests/test_tracking_rules.py feeds every rule the checker's own answer and one corruption per output.
  * the input builders those tests share (pose batches, alignment trials, seed batches, frame-pose cases).
"""
import collections
import functools
import math

import numpy as np

from helpers import FUZZ, camera_models, fuzz_rng
from oracle import pytrack
from rpg_svo_amd import se3, synth

N_LEVELS = 5
OK_SEED = (pytrack.SEED_UPDATED, pytrack.SEED_CONVERGED)
TOUCHED = (pytrack.SEED_NO_MATCH, pytrack.SEED_UPDATED, pytrack.SEED_CONVERGED, pytrack.SEED_NAN)   # statuses that write the seed
DEFAULT_SPREADS, DEFAULT_SEED_MIN = (0.4, 0.1, 0.0005), (0.6,)
CAP_SPREADS = (0.5, 0.25, 0.05)           # the queries of the search-step-cap test: lines on both sides of 6 and 20 steps
FILL = 77                                 # what a resident store holds where nobody wrote
FEATURE_KEYS = ("frame", "level", "type", "px", "f", "grad")          # (the member order of svo_hip_features)
SEED_KEYS = ("a", "b", "mu", "z_range", "sigma2", "batch_id")         # (the member order of svo_hip_seeds)
STATE_KEYS = ("a", "b", "mu", "sigma2")                               # the rows of the resident entry's dense read-back

# DepthFilter::updateSeed's a and b, device against CPU.  (e - f) / (f - e / f) cancels: a last-bit difference of an input
# comes out amplified.  Measured on 200 000 seeds with IDENTICAL float inputs (scripts/update_seed_parity.py on the GPU box,
# profiles/r04_update_seed_parity.json, the same against the C port and the reference's own translation unit): 99.98 % of
# the seeds come back with identical bits in all four fields (the rest: an exp that rounds the other way); largest
# relative deviation a 2.07e-5, b 2.04e-5, mu 1.7e-7, sigma2 1.7e-4 (a difference of two nearly equal products).
AB_RTOL_SAME_INPUTS = 1e-4   # 5 x the measured maximum
# In updateSeeds the inputs themselves (x = 1 / z, tau^2) come out of f64 geometry through acos / atan / sin, which can differ
# in the last bits between glibc and the GPU's libm before x is rounded to float.  Measured on the GPU box (the test prints
# it): 0.0 -- identical a and b -- on all 255 compared seeds of each of the six runs (3 option sets x 2 checkers).
AB_RTOL = 1e-4


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def feature_cols(fl):
    """[(frame, px, f, level, type, grad)] -> the six columns of a feature set"""
    return dict(frame=_c([o[0] for o in fl], np.int32), level=_c([o[3] for o in fl], np.int32), px=_c([o[1] for o in fl], np.float64),
                f=_c([o[2] for o in fl], np.float64), type=_c([o[4] for o in fl], np.uint8), grad=_c([o[5] for o in fl], np.float64))


def make_seeds(d_true, rng, seed_min=DEFAULT_SEED_MIN):
    """One seed per point as columns: depth d_true (1 + 0.1 N(0, 1)), depth_min = d_true * seed_min (cycled), a random batch
    id; every 7th at the convergence threshold (sigma = z_range / 227), every 31st with a negative mu, every 5th with
    sigma = z_range / 190 (a short epipolar segment)."""
    orc = pytrack.Track("orc")
    seeds = []
    for i in range(len(d_true)):
        s = orc.seed_init(d_true[i] * (1 + 0.1 * rng.normal()), d_true[i] * seed_min[i % len(seed_min)])
        s.batch_id = int(rng.integers(0, 6))
        if i % 7 == 0:
            s.sigma2 = np.float32(s.sigma2 * 7e-4)
        if i % 31 == 0:
            s.mu = np.float32(-0.3)
        if i % 5 == 0:
            s.sigma2 = np.float32(s.sigma2 * 1e-3)
        seeds.append(s)
    return {k: _c([getattr(x, k) for x in seeds], np.int32 if k == "batch_id" else np.float32) for k in SEED_KEYS}


class Queries:
    """epipolar queries on every `stride`-th point: feats, ftr_cols, d_est / d_min / d_max [n]"""

    def __init__(self, name, feats, d_true, rng, spreads, jitter, stride):
        self.name, self.feats = name, feats[::stride]
        self.n = len(self.feats)
        self.ftr_cols = feature_cols(self.feats)
        sp = np.array([spreads[k % len(spreads)] for k in range(self.n)])
        self.d_est = d_true[::stride] * (1 + rng.normal(size=self.n) * sp * jitter)
        self.d_min, self.d_max = self.d_est * (1 - sp), self.d_est * (1 + sp)


class Case:
    """scene: cam, T_f_w [K+1,12] (row `cur`: the current frame), images [K+1,h,w] u8, T_cur_prior, pt_pos [P,3], obs (per
    point: [(frame, px, f, level, type, grad)]), px_init [P,2].  feats: per point the feature of its seed / query; d_true [P]:
    its depth in that feature's frame.  rng: k -> Generator of the draws (fuzz_rng: SVO_TEST_FUZZ moves them)."""
    describe = staticmethod(lambda kind, i: None)   # (what an assert message says about entry i: track_edge_cases sets its classes)

    def __init__(self, name, scene, feats, d_true, spreads=DEFAULT_SPREADS, seed_min=DEFAULT_SEED_MIN, cap=None, stride=1, rng=fuzz_rng,
                 cam_kind=None, knobs=None):
        self.name, self.cam_kind, self.knobs, self.scene, self.cap = name, cam_kind, knobs, scene, cap
        self.images = np.ascontiguousarray(scene.images if isinstance(scene.images, np.ndarray) else scene.images.cpu().numpy())
        self.P, self.feats, self.d_true = len(scene.obs), feats, np.asarray(d_true)
        self._cache = {}
        T = scene.T_f_w.copy()
        T[scene.cur] = scene.T_cur_prior
        self.T_match, self.T_f_w = np.ascontiguousarray(T), np.ascontiguousarray(scene.T_f_w)
        self.obs_ptr = np.zeros(self.P + 1, np.int32)
        flat = []
        for i, o in enumerate(scene.obs):
            self.obs_ptr[i + 1] = self.obs_ptr[i] + len(o)
            flat.extend(o)
        self.obs_cols, self.ftr_cols = feature_cols(flat), feature_cols(feats)
        self.epi = Queries("epi", feats, self.d_true, rng(11), spreads, 0.3, stride)
        self.epi_cap = Queries("epi_cap", feats, self.d_true, rng(23), CAP_SPREADS, 0.2, stride)
        self.seed_cols = make_seeds(self.d_true, rng(8), seed_min)

    # -- the checker's answers, each computed once ----------------------------------------------------------------------------
    def _memo(self, key, fn):
        if key not in self._cache:
            self._cache[key] = fn()
        return self._cache[key]

    def checker(self, which):
        """-> (Track, pyramids, frames with the prior pose of the current frame, frames with the true one)"""
        def make():
            orc = pytrack.Track(which)
            pyrs = [orc.create_img_pyramid(im, N_LEVELS) for im in self.images]
            return orc, pyrs, pytrack.make_frames(pyrs, self.T_match), pytrack.make_frames(pyrs, self.scene.T_f_w)
        return self._memo(("checker", which), make)

    def matcher_ref(self, which="orc"):
        def run():
            orc, _, fm, _ = self.checker(which)
            s, opt = self.scene, pytrack.matcher_options(n_pyr_levels=N_LEVELS)
            return [orc.find_match_direct(fm, s.cam, s.cur, s.pt_pos[i], [pytrack.make_feature(*x) for x in s.obs[i]], s.px_init[i], opt)
                    for i in range(self.P)]
        return self._memo(("matcher", which), run)

    def epi_ref(self, which="orc", align_1d=0, cap=1000, q=None):
        q = q or self.epi

        def run():
            orc, _, _, ft = self.checker(which)
            s, opt = self.scene, pytrack.matcher_options(n_pyr_levels=N_LEVELS, align_1d=align_1d, max_epi_search_steps=cap)
            return [orc.find_epipolar_match_direct(ft, s.cam, q.feats[k][0], s.cur, pytrack.make_feature(*q.feats[k]), q.d_est[k],
                                                   q.d_min[k], q.d_max[k], opt) for k in range(q.n)]
        return self._memo((q.name, which, align_1d, cap), run)

    def seeds_ref(self, which="orc", align_1d=0, subpix=1, cap=1000):
        """-> (the seeds after DepthFilter::updateSeeds, the per-seed report), batch_counter = 5"""
        def run():
            orc, _, _, ft = self.checker(which)
            s, sc = self.scene, self.seed_cols
            seeds = []
            for i in range(self.P):
                sd = pytrack.Seed()
                sd.ftr = pytrack.make_feature(*self.feats[i])
                sd.batch_id, sd.a, sd.b, sd.mu = int(sc["batch_id"][i]), sc["a"][i], sc["b"][i], sc["mu"][i]
                sd.z_range, sd.sigma2 = sc["z_range"][i], sc["sigma2"][i]
                seeds.append(sd)
            opt = pytrack.matcher_options(n_pyr_levels=N_LEVELS, align_1d=align_1d, subpix_refinement=subpix, max_epi_search_steps=cap)
            _, so, io = orc.update_seeds(ft, s.cam, s.cur, seeds, batch_counter=5, opt=opt)
            return so, io
        return self._memo(("seeds", which, align_1d, subpix, cap), run)

    def pose_ref(self, which, ordered, row):
        """-> (pose_batch(scene, ordered, row), the checker's answer per frame)"""
        def run():
            batch = pose_batch(self.scene, ordered, row)
            return batch, pose_want(self.checker(which)[0], self.scene.cam, batch)
        return self._memo(("pose", which, ordered, row), run)


def of_scene(scene, name="scene", rng=fuzz_rng, cam_kind=None):
    """a synth.TrackScene as a case: a point's seed / query feature is its first observation outside the current frame, the
    queries take every second point"""
    feats, d_true = [], []
    for i in range(len(scene.obs)):
        o = [x for x in scene.obs[i] if x[0] != scene.cur][0]
        c_ref = -scene.T_f_w[o[0], :9].reshape(3, 3).T @ scene.T_f_w[o[0], 9:]
        feats.append(o)
        d_true.append(np.linalg.norm(scene.pt_pos[i] - c_ref))
    return Case(name, scene, feats, np.array(d_true), stride=2, rng=rng, cam_kind=cam_kind)


@functools.lru_cache(maxsize=None)
def committed(cam_kind):
    """the committed scene seen through each vikit camera model (undistorted pinhole, the reference's camera_pinhole.yaml with
    radial-tangential distortion, its camera_atan.yaml)"""
    scene = synth.make_track_scene(n_kf=4, n_feat=100, cam=camera_models()[cam_kind], seed=777 + FUZZ)
    return of_scene(scene, "committed", cam_kind=cam_kind)


# ---- the rules of the matcher and the depth filter -----------------------------------------------------------------------------
def verify_matcher(c, ok, px, ref_obs, sl, A, patches, which="orc"):
    """Matcher::findMatchDirect: verdict, chosen observation, search level, patch bytes and refined pixel identical, A_cur_ref
    to 1e-12 (f64 geometry).  ref_obs: index into the flattened observations.  Returns the largest |dA|."""
    worst = 0.0
    for i, (o_ok, o_px, r) in enumerate(c.matcher_ref(which)):
        assert bool(ok[i]) == o_ok, (c.name, i)
        assert ref_obs[i] - c.obs_ptr[i] == r["ref_obs"], (c.name, i)
        if r["A_cur_ref"].any():
            assert sl[i] == r["search_level"], (c.name, i, sl[i], r["search_level"])
            dA = np.abs(A[i].reshape(2, 2) - r["A_cur_ref"]).max()
            worst = max(worst, dA)
            assert dA < 1e-12, (c.name, i, dA)
            assert np.array_equal(patches[i], r["patch_with_border"]), (c.name, i, c.describe("matcher", i) if which == "orc" else None)
        assert np.array_equal(px[i], o_px), (c.name, i, px[i], o_px)
    return worst


def matcher_coverage(c, which="orc"):
    """-> (trials the checker matches, of those on an edgelet)"""
    res = c.matcher_ref(which)
    return sum(r[0] for r in res), sum(r[0] and c.scene.obs[i][r[2]["ref_obs"]][4] == 1 for i, r in enumerate(res))


def verify_epipolar(c, align_1d, cap, ok, depth, px, lvl, which="orc", q=None):
    """Matcher::findEpipolarMatchDirect: verdict and search level identical, px_cur to 1e-9, depth to 1e-9 relative.  Returns
    (largest |dpx|, largest relative depth difference)."""
    wpx = wd = 0.0
    for k, (ok_o, r) in enumerate(c.epi_ref(which, align_1d, cap, q)):
        assert bool(ok[k]) == ok_o, (c.name, k, ok[k], ok_o, c.describe("epi", k))
        if ok_o:
            assert lvl[k] == r["search_level"], (c.name, k)
            dpx, dd = np.abs(px[k] - r["px_cur"]).max(), abs(depth[k] - r["depth"]) / abs(r["depth"])
            wpx, wd = max(wpx, dpx), max(wd, dd)
            assert dpx < 1e-9 and dd < 1e-9, (c.name, k, dpx, dd, c.describe("epi", k))
    return wpx, wd


def verify_epipolar_cap(c, cap, ok_free, ok, depth, px, lvl, which="orc"):
    """Matcher::Options::max_epi_search_steps below the scan length (matcher.cpp:248-256: "skip epipolar search", `return
    false` before the first position is scored), on the queries c.epi_cap: those whose line is longer than `cap` steps fail
    and nothing of the match leaks out (depth 0), the others are untouched by the cap -- and the cap really fired (ok_free:
    the library's verdicts without it).  Returns (matched, cut by the cap)."""
    verify_epipolar(c, 0, cap, ok, depth, px, lvl, which, c.epi_cap)
    capped, free = c.epi_ref(which, 0, cap, c.epi_cap), c.epi_ref(which, 0, 1000, c.epi_cap)
    n_cut = 0
    for k in range(c.epi_cap.n):
        if not capped[k][0] and ok_free[k]:
            assert free[k][0], k  # the checker, too, matches this query without the cap: the cap is what failed it
            n_cut += 1
            assert depth[k] == 0.0, k
    n_ok = sum(r[0] for r in capped)
    assert n_cut >= 5 and n_ok >= 5, (n_cut, n_ok)
    return n_ok, n_cut


def _map_ref_status(status, which):
    """the reference's updateSeeds leaves no trace of "behind the camera" / "outside the image" (depth_filter.cpp:225-232:
    plain `continue`): its driver reports 0 for both"""
    return np.where(np.isin(status, (pytrack.SEED_BEHIND, pytrack.SEED_NOT_IN_FRAME)), 0, status) if which == "ref" else status


def _verify_status(status_i, st, so_i, tag):
    if st in OK_SEED:
        # the convergence test sqrt(sigma2) < z_range/200 is a float threshold: only demand the same verdict when the checker
        # is not sitting on it
        margin = abs(np.sqrt(max(so_i.sigma2, 0.0)) * 200.0 / so_i.z_range - 1.0)
        if margin > 1e-3:
            assert status_i == st, tag
        else:
            assert status_i in OK_SEED, tag
    else:
        assert status_i == st, tag


def verify_seeds(c, align_1d, subpix, cap, status, a, b, mu, s2, xyz, px, *_, which="orc", device=False):
    """DepthFilter::updateSeeds.  Statuses identical (off the convergence threshold); mu to 2e-6 relative; a / b to AB_RTOL;
    px_cur to 1e-9 ("orc" only: the reference's DepthFilter does not expose Matcher::px_cur_ per seed); a converged seed's
    point to 1e-5.  sigma2 is formed as C1*(s2+m^2) + C2*(sigma2+mu^2) - mu_new^2 in float: a last-bit difference of its
    inputs (an f64 depth through the algebraic computeTau, exp) shows as ~eps32 * mu^2 ABSOLUTE whatever sigma2's size.
    device=True: 4 eps32 (sigma2 + mu^2), what one last-bit input difference could cause (MEASURED on the GPU: 0 on the
    committed scene, three cameras x three option sets x both checkers; SVO_TEST_FUZZ=1..8, profiles/r06ad_*: up to 6.1
    eps32 mu^2 on other scenes -- 1.4e-5 of sigma2 -- hence 16 eps32 there); device=False, the emulation: 1e-4 sigma2 +
    1e-6 mu^2.  Returns the largest deviations: mu, sigma2, ab relative, px absolute, sigma2 in units of eps32 mu^2 (s2_eps),
    and the number of seeds whose a / b were compared (n_ab)."""
    so, io = c.seeds_ref(which, align_1d, subpix, cap)
    status = _map_ref_status(status, which)
    w = dict(mu=0.0, sigma2=0.0, ab=0.0, px=0.0, s2_eps=0.0, n_ab=0)
    for i in range(c.P):
        st = io[i].status
        tag = (c.name, i, int(status[i]), st)
        _verify_status(status[i], st, so[i], tag)
        # (a converged seed is erased from the reference's list; its driver recovers mu and sigma2 AFTER the last update
        #  from what the converged callback is handed -- the variance, and the new point, whose distance from the seed's
        #  frame is 1 / mu -- while a and b leave no trace there; the C port reports all four)
        ab_known = not (which == "ref" and st == pytrack.SEED_CONVERGED)
        if st in (pytrack.SEED_UPDATED, pytrack.SEED_CONVERGED, pytrack.SEED_NO_MATCH):
            assert np.isclose(mu[i], so[i].mu, rtol=2e-6, atol=0), (tag, mu[i], so[i].mu)
            ds2 = abs(float(s2[i]) - so[i].sigma2)
            if device:
                assert ds2 <= (9.6e-7 if FUZZ else 2.4e-7) * (abs(so[i].sigma2) + so[i].mu ** 2), (tag, s2[i], so[i].sigma2)
            else:
                assert ds2 <= 1e-4 * abs(so[i].sigma2) + 1e-6 * so[i].mu ** 2, (tag, s2[i], so[i].sigma2)
            if so[i].mu != 0:
                w["mu"] = max(w["mu"], abs(float(mu[i]) - so[i].mu) / abs(so[i].mu))
            if so[i].sigma2 != 0:
                w["sigma2"] = max(w["sigma2"], ds2 / abs(so[i].sigma2))
            if so[i].sigma2 != 0 and so[i].mu != 0:
                w["s2_eps"] = max(w["s2_eps"], ds2 / (6e-8 * so[i].mu ** 2))
            if ab_known:
                w["n_ab"] += 1
                w["ab"] = max(w["ab"], abs(float(a[i]) - so[i].a) / abs(so[i].a), abs(float(b[i]) - so[i].b) / abs(so[i].b))
                assert np.allclose([a[i], b[i]], [so[i].a, so[i].b], rtol=AB_RTOL, atol=1e-5), (tag, a[i], so[i].a, b[i], so[i].b)
        if st in OK_SEED and which == "orc":
            dpx = np.abs(px[i] - np.array(io[i].px_cur[:])).max()
            w["px"] = max(w["px"], dpx)
            assert dpx < 1e-9, (tag, dpx)
        if st == pytrack.SEED_CONVERGED:
            assert np.abs(xyz[i] - np.array(io[i].xyz_world[:])).max() < 1e-5, tag
    return w


def format_deviations(w):
    return ", ".join(f"{k} {w[k]:.2e}" for k in ("mu", "sigma2", "ab", "px"))


def seed_coverage(c, which="orc", align_1d=0, subpix=1):
    """the committed scene reaches every outcome of updateSeeds: asserts the checker's histogram of statuses"""
    hist = collections.Counter(x.status for x in c.seeds_ref(which, align_1d, subpix)[1])
    assert hist[pytrack.SEED_UPDATED] > 50 and hist[pytrack.SEED_CONVERGED] > 2, hist
    assert hist[pytrack.SEED_ERASED_OLD] > 5 and hist[pytrack.SEED_BEHIND if which == "orc" else 0] > 2, hist


def verify_seeds_cap(c, cap, status_free, status, a, b, mu, s2, *_, which="orc"):
    """DepthFilter::updateSeeds with Matcher::Options::max_epi_search_steps = cap: a seed whose line is longer is a failed
    match (b + 1 and nothing else, depth_filter.cpp:238-242), everything else as without the cap; statuses and seed state
    like the checker's.  status_free: the library's statuses without the cap.  Returns the number of seeds the cap cut."""
    so, io = c.seeds_ref(which, 0, 1, cap)
    status = _map_ref_status(status, which)
    b_before = c.seed_cols["b"]
    n_cut = 0
    for i in range(c.P):
        st = io[i].status
        _verify_status(status[i], st, so[i], (c.name, i, int(status[i]), st))
        if st == pytrack.SEED_NO_MATCH:
            assert b[i] == np.float32(b_before[i] + np.float32(1.0)) and b[i] == np.float32(so[i].b), i
            assert a[i] == np.float32(so[i].a) and mu[i] == np.float32(so[i].mu) and s2[i] == np.float32(so[i].sigma2), i
            if status_free[i] in OK_SEED:
                n_cut += 1
        elif st == pytrack.SEED_UPDATED:
            assert np.isclose(mu[i], so[i].mu, rtol=2e-6, atol=0), i
    assert n_cut >= 5, n_cut
    return n_cut


def seed_order(c):
    """The seeds keyframe by keyframe, as a seed list holds them: a wave of seed_prepare_kernel then finds a handful of runs of
    equal (reference, current) pairs whose first seed files the pair's poses for seed_finish; in list order the keyframe
    changes from seed to seed -- nearly every seed a run of its own."""
    fr = c.ftr_cols["frame"]
    order = np.argsort(fr, kind="stable")
    assert np.count_nonzero(np.diff(fr) != 0) > 64 > np.count_nonzero(np.diff(fr[order]) != 0)
    return order


def verify_seed_order(order, first, second, which="orc"):
    """the run on the seeds in keyframe order gives the bits of the run in list order.  first, second: what a backend's
    update_seeds returns (status, a, b, mu, sigma2, xyz, px, and the columns it leaves alone where the backend has them);
    xyz where the seed converged"""
    st1, st2 = _map_ref_status(first[0], which), _map_ref_status(second[0], which)
    assert np.array_equal(st2, st1[order])
    conv = st1[order] == pytrack.SEED_CONVERGED
    assert np.array_equal(second[5][conv], first[5][order][conv])
    for k in [k for k in range(1, len(first)) if k != 5]:
        assert np.array_equal(second[k], first[k][order]), k


def resident_slots(c):
    """the slots of the case's seeds in a store of 3 P slots (the draws that follow the seeds' own)"""
    rng = fuzz_rng(8)
    make_seeds(c.d_true, rng)
    return rng.permutation(3 * c.P)[:c.P].astype(np.int32)


def verify_resident(slots, n_slots, flat, resident, by_pose=None):
    """Row N2, seeds: the seeds scattered over the slots of a resident store (svo_hip_seed_store_patch) and updated through
    svo_hip_update_seeds_resident in list order: statuses, new points, px_cur and the state -- in the store AND in the dense
    read-back -- are the bits svo_hip_update_seeds produces on the flattened list (bit patterns: NaN seeds included); slots
    nobody named are untouched.  flat: (status, xyz, px, seed columns after the run); resident, by_pose: (status, xyz, px,
    state [4,S], the store's seed columns, the store's feature columns); by_pose: the same through
    svo_hip_update_seeds_resident_pose on a second store.  Returns (seeds written, seeds converged)."""
    (st0, xyz0, px0, cols0), (st1, xyz1, px1, state, store_s, store_f) = flat, resident
    assert np.array_equal(st0, st1) and np.array_equal(px0, px1)
    conv = st0 == pytrack.SEED_CONVERGED
    assert np.array_equal(xyz0[conv], xyz1[conv])
    touched = np.isin(st0, TOUCHED)
    bits = lambda x: np.ascontiguousarray(x).view(np.int32)
    for k, name in enumerate(STATE_KEYS):
        assert np.array_equal(bits(cols0[name]), bits(store_s[name][slots])), name
        assert np.array_equal(bits(state[k][touched]), bits(cols0[name][touched])), name
    free = np.ones(n_slots, bool)
    free[slots] = False
    assert (store_s["mu"][free] == FILL).all() and (store_f["level"][free] == FILL).all() and (store_s["batch_id"][free] == FILL).all()
    if by_pose is not None:
        st2, xyz2, px2, state2, store_s2, _ = by_pose
        assert np.array_equal(st2, st1) and np.array_equal(px2, px1) and np.array_equal(xyz2[conv], xyz1[conv])
        assert np.array_equal(bits(state2[:, touched]), bits(state[:, touched]))
        for name in STATE_KEYS:
            assert np.array_equal(bits(store_s2[name]), bits(store_s[name])), name
    return int(touched.sum()), int(conv.sum())


# ---- feature alignment ---------------------------------------------------------------------------------------------------
def align_trials(pyrs, rng, M, reach):
    """M random trials: a frame and a level, the 10 x 10 template from the same place in the same or the neighbouring frame,
    the start up to `reach` px off; every 37th start leaves the image, every 41st template is flat (singular H -> NaN)"""
    n = len(pyrs)
    slot = rng.integers(0, n, size=M).astype(np.int32)
    level = rng.integers(0, 3, size=M).astype(np.int32)
    pwb, px0 = np.zeros((M, 100), np.uint8), np.zeros((M, 2))
    dirs = rng.normal(size=(M, 2)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    use_1d = (rng.uniform(size=M) < 0.3).astype(np.uint8)
    for t in range(M):
        h, w = pyrs[slot[t]][level[t]].shape
        u, v = rng.integers(8, w - 8), rng.integers(8, h - 8)
        src = pyrs[(slot[t] + (t % 2)) % n][level[t]]
        pwb[t] = src[v - 5:v + 5, u - 5:u + 5].ravel()
        px0[t] = [u + rng.uniform(-reach, reach), v + rng.uniform(-reach, reach)]
        if t % 37 == 0:
            px0[t] = [3.0 + rng.uniform(0, 2), v]
        if t % 41 == 0:
            pwb[t] = 77
    return dict(slot=slot, level=level, pwb=pwb, px0=px0, dirs=dirs, use_1d=use_1d)


def check_alignment(orc, pyrs, tr, n_iter, ok, px, h_inv, every=1):
    """align1D / align2D of the reference on every `every`-th trial: verdict, refined pixel and (1-D) h_inv identical, NaN and
    infinity included.  Returns the number of compared trials that converged."""
    n_conv = 0
    for t in range(0, len(ok), every):
        img = pyrs[tr["slot"][t]][tr["level"][t]]
        patch = tr["pwb"][t].reshape(10, 10)[1:9, 1:9].ravel()
        if tr["use_1d"][t]:
            o, p, hi = orc.align1d(img, tr["dirs"][t], tr["pwb"][t], patch, n_iter, tr["px0"][t])
            assert hi == h_inv[t] or (np.isnan(hi) and np.isnan(h_inv[t])) or (np.isinf(hi) and np.isinf(h_inv[t])), (t, hi, h_inv[t])
        else:
            o, p = orc.align2d(img, tr["pwb"][t], patch, n_iter, tr["px0"][t])
        assert bool(ok[t]) == o, (t, n_iter)
        assert np.array_equal(p, px[t], equal_nan=True), (t, n_iter, p, px[t])
        n_conv += o
    return n_conv


def same_alignment(a, b, n=None):
    """two alignment runs (px, ok, h_inv[, evaluations]) with the same bits in their first n trials"""
    for k, (x, y) in enumerate(zip(a, b)):
        x, y = np.ascontiguousarray(x[:n]), np.ascontiguousarray(y[:n])
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint64 if x.dtype == np.float64 else x.dtype),
                                                     y.view(np.uint64 if y.dtype == np.float64 else y.dtype)), k


# ---- pose optimizer ------------------------------------------------------------------------------------------------------
def pose_batch(scene, ordered, row):
    """Twelve frames on the scene's points, observed 0.3 px off with every 15th point grossly wrong (pruning fires), 80 % of
    the observations live, frame 9 without any; n from 1 to all.  The wave kernel takes rows of up to 256 observations
    (svo_track::POSE_WAVE_MAX_STRIDE; a longer row goes to the ordered kernel whatever the entry): its legs are given 250, 128
    and 64 of the scene's 400 points -- the kernel's instantiations with four, two and one observation per lane; the drop-in's
    frames of ~120 matches run the second.  A batch: ns, n [B], f [B,ns,3], level [B,ns], pos [B,ns,3], hp [B,ns], T0 [B,12]."""
    rng = fuzz_rng(2)
    P = len(scene.pt_pos) if ordered else min(len(scene.pt_pos), row)
    B = 12
    f = synth._bearing(scene.cam, scene.px_true[:P] + rng.normal(size=(P, 2)) * 0.3)
    level = rng.integers(0, 3, size=P).astype(np.int32)
    pos = scene.pt_pos[:P].copy()
    pos[::15] += rng.normal(size=pos[::15].shape) * 0.2
    n = np.minimum(np.array([P, 200, 120, 40, 7, 3, P, P, 1, 150, 64, 5], dtype=np.int32), P).astype(np.int32)
    hp = (rng.uniform(size=(B, P)) > 0.2).astype(np.uint8)
    hp[9] = 0
    T0 = np.stack([se3.mul(se3.exp(rng.normal(size=6) * 5e-3), scene.T_f_w[scene.cur]) for _ in range(B)])
    return dict(ns=P, n=n, f=np.tile(f, (B, 1, 1)), level=np.tile(level, (B, 1)), pos=np.tile(pos, (B, 1, 1)), hp=hp, T0=T0)


def pose_deferred_batch(scene):
    """six frames of at most 200 observations (<= 256 per frame: the wave kernel's range), every one live; n = 2 and n = 1 are
    singular"""
    rng = fuzz_rng(4)
    P = min(len(scene.pt_pos), 200)
    B = 6
    f = synth._bearing(scene.cam, scene.px_true[:P] + rng.normal(size=(P, 2)) * 0.3)
    level = rng.integers(0, 3, size=P).astype(np.int32)
    n = np.array([P, 150, 2, 64, 1, 40], dtype=np.int32)
    T0 = np.stack([se3.mul(se3.exp(rng.normal(size=6) * 5e-3), scene.T_f_w[scene.cur]) for _ in range(B)])
    return dict(ns=P, n=n, f=np.tile(f, (B, 1, 1)), level=np.tile(level, (B, 1)), pos=np.tile(scene.pt_pos[:P], (B, 1, 1)),
                hp=np.ones((B, P), dtype=np.uint8), T0=T0)


def pose_want(orc, cam, batch, n_iter=10, thresh=2.0):
    n = batch["n"]
    return [orc.pose_optimize(cam, batch["T0"][b], batch["f"][b, :n[b]], batch["level"][b, :n[b]], batch["hp"][b, :n[b]],
                              batch["pos"][b, :n[b]], thresh, n_iter) for b in range(len(n))]


def check_pose(n, hp, T0, want, T, Cov, stats, ran, hp_out, ordered=False, beyond_n=False, tight_stats_live=20, what=None):
    """pose_optimizer::optimizeGaussNewton, frame by frame against the checker's answers `want`.
    ordered=True: the checker kernel (normal equations summed in the reference's order; what differs is sin / cos in
    SE3::exp): the pose (SE(3) log norm) to 1e-10.  ordered=False: the pipeline's wave kernel: 2e-8 per frame with 20 or
    more live observations, 1e-7 below; identical pruning decisions and observation counts; frames whose normal equations
    are singular are handed to the ordered kernel and therefore still match.
      (wave kernel: 1e-15 on frames of 28 ... 250 observations, measured; five to seven live observations -- ten to fourteen
       equations for six unknowns under Tukey weights -- amplify the summation order to 3e-9 ... 6e-9 on three of twenty
       scenes; the pipeline gives up on a frame with fewer than Config::qualityMinFts = 50 features.  One frame of 48
       observations: 1.9e-9 -- at convergence chi2 moves in its last bits and "the error increased" is decided by rounding on
       both sides; a decision that falls the other way leaves the size of the last Gauss-Newton step.  Hence 2e-8 per frame,
       and the MEDIAN over a batch's well-posed frames at 1e-12: check_pose_median.)
    Scale and errors to 1e-9 relative where the pose agrees to 1e-11 on a frame of at least tight_stats_live live
    observations, else 1e-6 (the final error is the final pose's).  Cov to 1e-6 on a well-conditioned system: n >= 40 with at
    least three live observations (Cov is the inverse of the 6x6 normal matrix, whose rank is at most twice the number of
    live observations: below three of them it is singular and its "inverse" rounding noise of magnitude 1e13 on every side).
    beyond_n: the flags beyond a frame's n come back untouched.  Under SVO_TEST_FUZZ a frame with fewer than six live
    observations (normal equations of rank < 6 or nearly so, where the reference's own answer is decided by the rounding
    inside Eigen's pivoted LDLT) only has to have run and returned a pose on both sides.
    Returns the deviations of the frames with 20 or more live observations."""
    devs = []
    for b, o in enumerate(want):
        tag = (b, what[b] if what else None)
        assert ran[b] == o["ran"], tag
        if beyond_n:
            assert np.array_equal(hp_out[b, n[b]:], hp[b, n[b]:]), tag
        if not o["ran"]:
            assert np.array_equal(T[b], T0[b]) and np.array_equal(hp_out[b], hp[b]), tag
            continue
        live = int(hp[b, :n[b]].sum())
        if FUZZ and live < 6:
            assert np.isfinite(T[b]).all() == np.isfinite(o["T_f_w"]).all(), tag
            continue
        dev_b = se3.log_norm(T[b][None], o["T_f_w"][None])[0]
        if live >= 20:
            devs.append(dev_b)
        assert dev_b < (1e-10 if ordered else (2e-8 if live >= 20 else 1e-7)), (tag, dev_b)
        assert np.array_equal(hp_out[b, :n[b]], o["has_point"]), tag
        assert stats[b, 3] == o["num_obs"], tag
        tight = ordered or (live >= tight_stats_live and dev_b < 1e-11)
        assert np.allclose(stats[b, :3], [o["estimated_scale"], o["error_init"], o["error_final"]], rtol=1e-9 if tight else 1e-6,
                           atol=1e-12), (tag, dev_b)
        if n[b] >= 40 and live >= 3:
            assert np.allclose(Cov[b].reshape(6, 6), o["Cov"], rtol=1e-6, atol=1e-14), tag
    return devs


def check_pose_median(devs):
    assert np.median(devs) < 1e-12, devs


def check_pose_batch(scene, batch, want, got, ordered):
    """check_pose on a pose_batch, the median, and frame 0 against the ground truth (the scene's noise)"""
    n, hp = batch["n"], batch["hp"]
    # (no frame of this batch has n >= 40 and one or two live observations: check_pose's Cov condition selects the frames
    #  that "n >= 40" alone selects)
    assert not any(n[b] >= 40 and 0 < int(hp[b, :n[b]].sum()) < 3 for b in range(len(n)))
    devs = check_pose(n, hp, batch["T0"], want, *got, ordered=ordered)
    check_pose_median(devs)
    P = batch["ns"]
    bound = (1.5e-2 if P >= 250 else 5e-2) if FUZZ else (2e-3 if P >= 250 else 5e-3)
    assert se3.log_norm(got[0][0][None], scene.T_f_w[scene.cur][None])[0] < bound
    return devs


def check_pose_deferred(batch, run):
    """svo_hip_pose_optimize_deferred = svo_hip_pose_optimize without the fix-up launch: same results on the frames the wave
    kernel takes; the others come back untouched with ran == 2 and are finished by svo_hip_pose_optimize_ordered.  n_iter = 0
    is a documented hand-over (the kernel only reports the initial error there), so it exercises that path for every frame.
    run(n_iter, entry) -> (T, Cov, stats, ran, has_point); entry: "", "_deferred" or "_ordered"."""
    T0, hp = batch["T0"], batch["hp"]
    Tf, _, _, ran_f, hp_f = run(10, "")
    Tp, _, _, ran_p, hp_p = run(10, "_deferred")
    assert not (ran_f == 2).any()
    taken = ran_p != 2
    assert taken.any()
    assert np.array_equal(Tf[taken], Tp[taken]) and np.array_equal(ran_f[taken], ran_p[taken]) and np.array_equal(hp_f[taken], hp_p[taken])
    assert np.array_equal(Tp[~taken], T0[~taken]) and np.array_equal(hp_p[~taken], hp[~taken])          # untouched
    # n_iter = 0: everything is handed over; the caller's second step gives what the one-call entry gives
    T0f, _, st0f, ran0f, hp0f = run(0, "")
    T0p, _, _, ran0p, hp0p = run(0, "_deferred")
    assert (ran0p == 2).all() and np.array_equal(T0p, T0) and np.array_equal(hp0p, hp)
    T0o, _, st0o, ran0o, hp0o = run(0, "_ordered")
    assert np.array_equal(T0o, T0f) and np.array_equal(ran0o, ran0f) and np.array_equal(hp0o, hp0f) and np.array_equal(st0o, st0f)


# ---- point optimizer, reprojection, match selection, seed batches -------------------------------------------------------------
def point_optimize_inputs(scene):
    """-> (obs_ptr, frame per observation, bearings 1e-3 off, start positions 0.05 off)"""
    rng = fuzz_rng(4)
    ptr = np.zeros(len(scene.obs) + 1, dtype=np.int32)
    fr, ff = [], []
    for i, o in enumerate(scene.obs):
        ptr[i + 1] = ptr[i] + len(o)
        for x in o:
            fr.append(x[0])
            ff.append(x[2] + rng.normal(size=3) * 1e-3)
    p0 = scene.pt_pos + rng.normal(size=scene.pt_pos.shape) * 0.05
    return ptr, np.array(fr, np.int32), _c(ff, np.float64), np.ascontiguousarray(p0)


def check_point_optimize(orc, scene, ptr, ff, p0, out):
    """Point::optimize (five iterations) on every third point: 1e-11"""
    for i in range(0, len(scene.obs), 3):
        T = np.array([scene.T_f_w[x[0]] for x in scene.obs[i]])
        o = orc.point_optimize(T, ff[ptr[i]:ptr[i + 1]], p0[i], 5)
        assert np.abs(o - out[i]).max() < 1e-11, i


def check_reproject_points(orc, scene, cell, px):
    """the grid cell (30 px, 22 columns) identical, the pixel to 1e-10; more than half of the points land in the image"""
    P = len(scene.pt_pos)
    for i in range(P):
        k, p = orc.reproject_point(scene.cam, scene.T_f_w[scene.cur], scene.pt_pos[i], 30, 22)
        assert k == cell[i] and np.abs(p - px[i]).max() < 1e-10
    assert (cell >= 0).sum() > P // 2


SELECT_SHAPES_DEVICE = ((0, 120), (1, 120), (7, 0), (130, 120), (300, 120), (300, 40), (1500, 120), (1500, 10000), (5000, 700))
SELECT_SHAPES_EMULATED = ((0, 120), (1, 120), (7, 0), (130, 120), (300, 40), (1500, 120), (1500, 10000))


def select_trials(cam, rng, M):
    """M trials in runs of 1 to 8 per cell, 45 % matched -> (cell, ok, px, level, pos)"""
    runs = rng.integers(1, 9, size=M + 1)
    cell = np.repeat(rng.permutation(M + 1), runs)[:M].astype(np.int32)
    ok = (rng.uniform(size=M) < 0.45).astype(np.int32)
    px = np.ascontiguousarray(np.stack([rng.uniform(0, cam.width, M), rng.uniform(0, cam.height, M)], axis=1).reshape(M, 2))
    return cell, ok, px, rng.integers(0, 4, size=M).astype(np.int32), rng.normal(size=(M, 3))


def check_select_matches(cam, trials, max_fts, n, sel, f, lvl, p, has):
    """svo_hip_select_matches against the restated cell loop of Reprojector::reprojectMap (reprojector.cpp:131-139, 150-200):
    which trials become features, in which order, and the observation each one hands to the pose optimizer.  Indices / levels
    / positions identical; the bearing within 1e-14 (device tan / sqrt of the ATAN model)."""
    sel_o, f_o, lvl_o, pos_o = pytrack.select_matches(cam, *trials, max_fts)
    k = int(n)
    assert k == len(sel_o)
    assert np.array_equal(sel[:k], sel_o) and np.array_equal(lvl[:k], lvl_o)
    assert np.array_equal(p[:k], pos_o) and bool((has[:k] == 1).all())
    if k:
        assert np.abs(f[:k] - f_o).max() <= 1e-14


def seed_batch(orc, rng, S):
    """S seeds with a, b in 5 ... 30 and one measurement each; every 50th with tau2 = 0, every 77th far off (x = 50)
    -> (the checker's seeds, their columns, x, tau2)"""
    seeds = []
    for i in range(S):
        s = orc.seed_init(rng.uniform(0.5, 5), rng.uniform(0.2, 0.5))
        s.a, s.b = np.float32(rng.uniform(5, 30)), np.float32(rng.uniform(5, 30))
        seeds.append(s)
    x = (1.0 / rng.uniform(0.5, 5, size=S)).astype(np.float32)
    tau2 = (10.0 ** rng.uniform(-8, 0, size=S)).astype(np.float32)
    tau2[::50] = 0.0
    x[::77] = 50.0
    cols = {k: _c([getattr(s, k) for s in seeds], np.float32) for k in SEED_KEYS[:5]}
    cols["batch_id"] = np.zeros(S, np.int32)
    return seeds, cols, x, tau2


def check_seed_batch(orc, seeds, x, tau2, cols, min_identical=0.0):
    """DepthFilter::updateSeed per seed: the same seeds finite; mu to 2e-6, sigma2 to 1e-4 sigma2 + 1e-6 mu^2, a / b to
    AB_RTOL_SAME_INPUTS (expf differs by an ulp between glibc and the GPU; a / b amplify it: (e-f)/(f-e/f) cancels).
    min_identical: the share of seeds with the checker's bits in all four fields."""
    got = np.stack([cols[k] for k in STATE_KEYS], axis=1).astype(np.float64)
    want = np.array([[n.a, n.b, n.mu, n.sigma2] for n in (orc.update_seed(x[i], tau2[i], seeds[i]) for i in range(len(seeds)))])
    fin = np.isfinite(want).all(axis=1)
    assert np.array_equal(np.isfinite(got).all(axis=1), fin)
    g, w = got[fin], want[fin]
    assert np.mean(np.all(g == w, axis=1)) >= min_identical
    assert np.allclose(g[:, 2], w[:, 2], rtol=2e-6, atol=0)
    assert (np.abs(g[:, 3] - w[:, 3]) <= 1e-4 * np.abs(w[:, 3]) + 1e-6 * w[:, 2] ** 2).all()
    assert np.allclose(g[:, :2], w[:, :2], rtol=AB_RTOL_SAME_INPUTS, atol=0)


# ---- svo_hip_frame_pose_compose: the host's side, statement for statement -------------------------------------------------------
def _quat_of(T12):
    """unit quaternion the host's SE3(R, t) constructor derives (oracle/orc_math.h: orc_quat_from_R)"""
    R = [float(x) for x in T12[:9]]
    tr = R[0] + R[4] + R[8]
    q = [0.0] * 4
    if tr > 0.0:
        s = math.sqrt(tr + 1.0)
        q[0] = 0.5 * s
        s = 0.5 / s
        q[1] = (R[7] - R[5]) * s; q[2] = (R[2] - R[6]) * s; q[3] = (R[3] - R[1]) * s
    else:
        i = 0
        if R[4] > R[0]: i = 1
        if R[8] > R[i * 3 + i]: i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        s = math.sqrt(R[i * 3 + i] - R[j * 3 + j] - R[k * 3 + k] + 1.0)
        q[1 + i] = 0.5 * s
        s = 0.5 / s
        q[0] = (R[k * 3 + j] - R[j * 3 + k]) * s
        q[1 + j] = (R[j * 3 + i] + R[i * 3 + j]) * s
        q[1 + k] = (R[k * 3 + i] + R[i * 3 + k]) * s
    return q


def _quat_product(q, b):
    """q * b, normalised (orc_se3_compose)"""
    w = q[0] * b[0] - q[1] * b[1] - q[2] * b[2] - q[3] * b[3]
    x = q[0] * b[1] + q[1] * b[0] + q[2] * b[3] - q[3] * b[2]
    y = q[0] * b[2] + q[2] * b[0] + q[3] * b[1] - q[1] * b[3]
    z = q[0] * b[3] + q[3] * b[0] + q[1] * b[2] - q[2] * b[1]
    n = math.sqrt(w * w + x * x + y * y + z * z)
    return [w / n, x / n, y / n, z / n]


def composed_quat(T_cur_ref, q_ref):
    """the unit quaternion of SE3(R, t) * T_ref before it is turned into a matrix (what Frame::isVisible rotates with)"""
    return _quat_product(_quat_of(T_cur_ref), [float(x) for x in q_ref])


def host_frame_pose(T_cur_ref, q_ref, t_ref):
    """poseToRt(SE3(R, t) * T_ref) as the host forms it (oracle/orc_math.h: orc_quat_from_R, orc_se3_compose, orc_quat_to_R),
    statement for statement in Python floats (IEEE doubles, no contraction): the bits svo_hip_frame_pose_compose must give."""
    t = [float(x) for x in T_cur_ref[9:]]
    q = _quat_of(T_cur_ref)
    v = [float(x) for x in t_ref]
    ux = q[2] * v[2] - q[3] * v[1]; uy = q[3] * v[0] - q[1] * v[2]; uz = q[1] * v[1] - q[2] * v[0]
    ux += ux; uy += uy; uz += uz
    cx = q[2] * uz - q[3] * uy; cy = q[3] * ux - q[1] * uz; cz = q[1] * uy - q[2] * ux
    rt = [v[0] + q[0] * ux + cx, v[1] + q[0] * uy + cy, v[2] + q[0] * uz + cz]
    to = [t[0] + rt[0], t[1] + rt[1], t[2] + rt[2]]
    w, x, y, z = _quat_product(q, [float(x) for x in q_ref])
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx,
                     1.0 - (txx + tyy)] + to)


def frame_pose_compose_cases(rng, n=200):
    """(T_cur_ref [12], q_ref [4], t_ref [3]) with rotations in every branch of the matrix -> quaternion conversion"""
    cases = []
    for i in range(n):
        big = i % 4 == 0  # rotations beyond 120 degrees: trace <= 0
        T = se3.exp(rng.normal(size=6) * (2.5 if big else 0.05))
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        cases.append((np.ascontiguousarray(T), q, rng.normal(size=3) * 3.0))
    return cases


def host_keyframe_ranks(cam, T12, q_cur, key_pos, key_valid, table, n_kf, max_n_kfs):
    """Map::getCloseKeyframes + the reprojector's stable closest-first sort and cut, in Python floats: per frame-table entry the
    rank or -1.  T12: the composed (R | t); q_cur: its unit quaternion (w, x, y, z) as the SE3 object holds it."""
    w, x, y, z = [float(v) for v in q_cur]
    t = [float(v) for v in T12[9:]]
    dist = [-1.0] * len(table)
    for i in range(n_kf):
        for k in range(5):
            if not key_valid[i, k]:
                continue
            v = [float(c) for c in key_pos[i, k]]
            ux = y * v[2] - z * v[1]; uy = z * v[0] - x * v[2]; uz = x * v[1] - y * v[0]
            ux += ux; uy += uy; uz += uz
            cx = y * uz - z * uy; cy = z * ux - x * uz; cz = x * uy - y * ux
            f = [(v[0] + w * ux + cx) + t[0], (v[1] + w * uy + cy) + t[1], (v[2] + w * uz + cz) + t[2]]
            if f[2] < 0.0:
                continue
            px = (cam.fx * (f[0] / f[2]) + cam.cx, cam.fy * (f[1] / f[2]) + cam.cy)  # (the undistorted pinhole)
            if px[0] >= 0.0 and px[1] >= 0.0 and px[0] < cam.width and px[1] < cam.height:
                d = [t[c] - float(table[i][9 + c]) for c in range(3)]
                dist[i] = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
                break
    ranks = []
    for i in range(len(table)):
        r = -1
        if dist[i] >= 0.0:
            r = sum(1 for j in range(n_kf) if dist[j] >= 0.0 and (dist[j] < dist[i] or (dist[j] == dist[i] and j < i)))
            if r >= max_n_kfs:
                r = -1
        ranks.append(r)
    return np.array(ranks, np.int32)


def keyframe_rank_case(rng, n_kf=12, n_tab=14):
    """a frame table of n_tab poses around the origin looking at points near z = 2, key points per keyframe (some missing, some
    behind / outside), two keyframes at EXACTLY the same distance (the stable order decides)"""
    table = np.stack([se3.exp(np.concatenate([rng.normal(size=3) * 0.3, rng.normal(size=3) * 0.05])) for _ in range(n_tab)])
    table[5, 9:] = table[3, 9:]  # equal translations -> equal distances
    key_pos = np.concatenate([rng.uniform(-2.5, 2.5, size=(n_kf, 5, 2)), rng.uniform(-1.0, 4.0, size=(n_kf, 5, 1))], axis=2)
    key_valid = (rng.uniform(size=(n_kf, 5)) < 0.8).astype(np.uint8)
    key_valid[7] = 0  # a keyframe without key points is never close
    return np.ascontiguousarray(table), np.ascontiguousarray(key_pos), key_valid
