"""The rules of tests/tracking_cases.py judged on their own, without a GPU and without the library under test: each rule
passes when it is fed the checker's own answer (the pinhole committed case, whose memoised answers the emulated tests of the
same session share) and fails on one targeted corruption per output.  What an emulated or a device test can pass is therefore
what these rules let through."""
import numpy as np
import pytest

import tracking_cases as tc
from helpers import FUZZ
from oracle import pytrack
from rpg_svo_amd import se3


@pytest.fixture(scope="module")
def case(oracle):
    return tc.committed("pinhole")


def fails(rule, *args, **kw):
    with pytest.raises(AssertionError):
        rule(*args, **kw)


def changed(arrays, k, index, value):
    """a copy of the tuple `arrays` with arrays[k][index] = value (a function of the old value, or a value)"""
    out = [np.array(a, copy=True) for a in arrays]
    out[k][index] = value(out[k][index]) if callable(value) else value
    return out


# ---- matcher ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def matcher_answer(case):
    res = case.matcher_ref()
    ok = np.array([r[0] for r in res], np.int32)
    px = np.array([r[1] for r in res], np.float64)
    ref_obs = case.obs_ptr[:-1] + np.array([r[2]["ref_obs"] for r in res], np.int32)
    sl = np.array([r[2]["search_level"] for r in res], np.int32)
    A = np.array([r[2]["A_cur_ref"].ravel() for r in res])
    patches = np.array([r[2]["patch_with_border"] for r in res], np.uint8)
    return ok, px, ref_obs, sl, A, patches


def test_matcher_rule(case, matcher_answer):
    assert tc.verify_matcher(case, *matcher_answer) == 0.0
    i = int(np.flatnonzero(matcher_answer[0])[3])          # a trial that matched: its warp was reached
    fails(tc.verify_matcher, case, *changed(matcher_answer, 0, i, 0))                                   # a flipped ok
    fails(tc.verify_matcher, case, *changed(matcher_answer, 2, i, lambda v: v + 1))                     # ref_obs off by one
    fails(tc.verify_matcher, case, *changed(matcher_answer, 3, i, lambda v: v + 1))                     # the search level
    fails(tc.verify_matcher, case, *changed(matcher_answer, 5, (i, 57), lambda v: v ^ 1))               # one patch byte
    fails(tc.verify_matcher, case, *changed(matcher_answer, 1, (i, 1), lambda v: np.nextafter(v, np.inf)))   # px by one ulp
    fails(tc.verify_matcher, case, *changed(matcher_answer, 4, (i, 2), lambda v: v + 2e-12))            # A off by 2e-12
    assert tc.verify_matcher(case, *changed(matcher_answer, 4, (i, 2), lambda v: v + 5e-13)) > 4e-13    # (inside the bound)


# ---- epipolar queries -----------------------------------------------------------------------------------------------------------
def epipolar_answer(res):
    ok = np.array([r[0] for r in res], np.int32)
    depth = np.array([r[1]["depth"] if r[0] else 0.0 for r in res])
    px = np.array([r[1]["px_cur"] for r in res], np.float64)
    lvl = np.array([r[1]["search_level"] for r in res], np.int32)
    return ok, depth, px, lvl


def test_epipolar_rule(case):
    ans = epipolar_answer(case.epi_ref("orc", 0, 1000))
    assert tc.verify_epipolar(case, 0, 1000, *ans) == (0.0, 0.0)
    k = int(np.flatnonzero(ans[0])[2])
    fails(tc.verify_epipolar, case, 0, 1000, *changed(ans, 0, k, 0))
    fails(tc.verify_epipolar, case, 0, 1000, *changed(ans, 1, k, lambda v: v * (1 + 2e-9)))             # depth off by 2e-9 relative
    fails(tc.verify_epipolar, case, 0, 1000, *changed(ans, 2, (k, 0), lambda v: v + 2e-9))
    fails(tc.verify_epipolar, case, 0, 1000, *changed(ans, 3, k, lambda v: v + 1))
    tc.verify_epipolar(case, 0, 1000, *changed(ans, 1, k, lambda v: v * (1 + 5e-10)))                   # (inside the bound)


def test_epipolar_cap_rule(case):
    cap = 6
    ok_free = epipolar_answer(case.epi_ref("orc", 0, 1000, case.epi_cap))[0]
    ans = epipolar_answer(case.epi_ref("orc", 0, cap, case.epi_cap))
    n_ok, n_cut = tc.verify_epipolar_cap(case, cap, ok_free, *ans)
    assert n_ok >= 5 and n_cut >= 5
    cut = int(np.flatnonzero((ans[0] == 0) & (ok_free != 0))[0])
    fails(tc.verify_epipolar_cap, case, cap, ok_free, *changed(ans, 1, cut, 1.5))                       # a match leaks out of a skipped search
    fails(tc.verify_epipolar_cap, case, cap, ok_free, *changed(ans, 0, cut, 1))
    fails(tc.verify_epipolar_cap, case, cap, np.zeros_like(ok_free), *ans)                              # the cap never fired


# ---- seeds ------------------------------------------------------------------------------------------------------------------
def seeds_answer(case, cap=1000):
    so, io = case.seeds_ref("orc", 0, 1, cap)
    f32 = lambda k: np.array([getattr(s, k) for s in so], np.float32)
    return (np.array([x.status for x in io], np.int32), f32("a"), f32("b"), f32("mu"), f32("sigma2"),
            np.array([x.xyz_world[:] for x in io]), np.array([x.px_cur[:] for x in io]))


def test_seeds_rule(case):
    ans = seeds_answer(case)
    so, io = case.seeds_ref("orc", 0, 1, 1000)
    for device in (False, True):
        w = tc.verify_seeds(case, 0, 1, 1000, *ans, device=device)
        assert w["mu"] == w["sigma2"] == w["ab"] == w["px"] == 0.0 and w["n_ab"] > 100
    margin = lambda i: abs(np.sqrt(max(so[i].sigma2, 0.0)) * 200.0 / so[i].z_range - 1.0)
    upd = next(i for i in range(case.P) if io[i].status == pytrack.SEED_UPDATED and margin(i) > 1e-3 and so[i].sigma2 > 0)
    conv = next(i for i in range(case.P) if io[i].status == pytrack.SEED_CONVERGED)
    for device in (False, True):
        rule = lambda *a: tc.verify_seeds(case, 0, 1, 1000, *a, device=device)
        fails(rule, *changed(ans, 0, upd, pytrack.SEED_CONVERGED))                                      # a status off the convergence margin
        fails(rule, *changed(ans, 0, upd, pytrack.SEED_NO_MATCH))
        fails(rule, *changed(ans, 3, upd, lambda v: v * np.float32(1 + 4e-6)))                          # mu off by 4e-6 relative
        fails(rule, *changed(ans, 1, upd, lambda v: v * np.float32(1 + 1e-3)))                          # a
        fails(rule, *changed(ans, 2, upd, lambda v: v * np.float32(1 + 1e-3) + np.float32(1e-4)))       # b
        fails(rule, *changed(ans, 6, (upd, 0), lambda v: v + 2e-9))                                     # px_cur
        fails(rule, *changed(ans, 5, (conv, 2), lambda v: v + 2e-5))                                    # a converged seed's point
    # sigma2 off by ten times its bound, under each rule separately
    s2, mu = so[upd].sigma2, so[upd].mu
    bound_device = (9.6e-7 if FUZZ else 2.4e-7) * (abs(s2) + mu ** 2)
    bound_emulated = 1e-4 * abs(s2) + 1e-6 * mu ** 2
    fails(tc.verify_seeds, case, 0, 1, 1000, *changed(ans, 4, upd, np.float32(s2 + 10 * bound_device)), device=True)
    fails(tc.verify_seeds, case, 0, 1, 1000, *changed(ans, 4, upd, np.float32(s2 + 10 * bound_emulated)), device=False)
    tc.verify_seeds(case, 0, 1, 1000, *changed(ans, 4, upd, np.float32(s2 + 0.5 * bound_device)), device=True)   # (inside)
    tc.verify_seeds(case, 0, 1, 1000, *changed(ans, 4, upd, np.float32(s2 + 0.5 * bound_emulated)), device=False)
    tc.seed_coverage(case)


def test_seeds_cap_rule(case):
    cap = 8
    free, ans = seeds_answer(case)[0], seeds_answer(case, cap)
    assert tc.verify_seeds_cap(case, cap, free, *ans) >= 5
    cut = int(np.flatnonzero((ans[0] == pytrack.SEED_NO_MATCH) & np.isin(free, tc.OK_SEED))[0])
    fails(tc.verify_seeds_cap, case, cap, free, *changed(ans, 2, cut, lambda v: v + np.float32(1)))     # b + 2
    fails(tc.verify_seeds_cap, case, cap, free, *changed(ans, 3, cut, lambda v: np.nextafter(v, np.float32(9))))   # and nothing else
    fails(tc.verify_seeds_cap, case, cap, free, *changed(ans, 0, cut, pytrack.SEED_UPDATED))
    fails(tc.verify_seeds_cap, case, cap, ans[0], *ans)                                                 # the cap never fired


def test_seed_order_rule(case):
    first = seeds_answer(case)
    order = tc.seed_order(case)
    second = tuple(x[order] for x in first)
    tc.verify_seed_order(order, first, second)
    k = int(np.flatnonzero(second[0] == pytrack.SEED_CONVERGED)[0])
    fails(tc.verify_seed_order, order, first, changed(second, 0, k, pytrack.SEED_UPDATED))
    fails(tc.verify_seed_order, order, first, changed(second, 3, k, lambda v: np.nextafter(v, np.float32(9))))
    fails(tc.verify_seed_order, order, first, changed(second, 5, (k, 0), lambda v: np.nextafter(v, 9.0)))
    fails(tc.verify_seed_order, order, first, changed(second, 6, (k, 1), lambda v: np.nextafter(v, 9e9)))


def test_resident_rule(case):
    st, a, b, mu, s2, xyz, px = seeds_answer(case)
    S, n_slots = case.P, 3 * case.P
    slots = tc.resident_slots(case)
    assert len(np.unique(slots)) == S and slots.max() < n_slots
    cols = dict(a=a, b=b, mu=mu, sigma2=s2)
    flat = (st, xyz, px, cols)

    def resident():
        store_s = {k: np.full(n_slots, tc.FILL, v.dtype) for k, v in case.seed_cols.items()}
        store_f = {k: np.full((n_slots,) + v.shape[1:], tc.FILL, v.dtype) for k, v in case.ftr_cols.items()}
        for k in store_s:
            store_s[k][slots] = cols.get(k, case.seed_cols[k])
        for k in store_f:
            store_f[k][slots] = case.ftr_cols[k]
        return [st.copy(), xyz.copy(), px.copy(), np.stack([cols[k] for k in tc.STATE_KEYS]), store_s, store_f]

    touched, conv = tc.verify_resident(slots, n_slots, flat, resident(), resident())
    assert touched > 100 and conv > 2
    free = int(np.setdiff1d(np.arange(n_slots), slots)[0])
    t = int(np.flatnonzero(np.isin(st, tc.TOUCHED))[0])
    for name, table in (("mu", 4), ("batch_id", 4), ("level", 5)):
        r = resident()
        r[table][name][free] = 1                                                                        # a slot outside `slots` overwritten
        fails(tc.verify_resident, slots, n_slots, flat, r)
    r = resident()
    r[4]["sigma2"][slots[t]] = np.nextafter(r[4]["sigma2"][slots[t]], np.float32(9))                    # the state in the store
    fails(tc.verify_resident, slots, n_slots, flat, r)
    r = resident()
    r[3][2, t] = np.nextafter(r[3][2, t], np.float32(9))                                                # the dense read-back
    fails(tc.verify_resident, slots, n_slots, flat, r)
    r = resident()
    r[0][t] = pytrack.SEED_NAN
    fails(tc.verify_resident, slots, n_slots, flat, r)
    r = resident()
    r[4]["a"][free] = 1                                                                                 # the second store differs from the first
    fails(tc.verify_resident, slots, n_slots, flat, resident(), r)


# ---- pose optimizer -------------------------------------------------------------------------------------------------------------
def pose_answer(batch, want):
    T, hp = batch["T0"].copy(), batch["hp"].copy()
    B = len(want)
    Cov, stats, ran = np.zeros((B, 36)), np.zeros((B, 4)), np.zeros(B, np.int32)
    for b, o in enumerate(want):
        ran[b] = o["ran"]
        if o["ran"]:
            T[b], Cov[b] = o["T_f_w"], np.asarray(o["Cov"]).ravel()
            stats[b] = [o["estimated_scale"], o["error_init"], o["error_final"], o["num_obs"]]
            hp[b, :batch["n"][b]] = o["has_point"]
    return T, Cov, stats, ran, hp


@pytest.mark.parametrize("ordered", [False, True])
def test_pose_rule(case, ordered):
    batch, want = case.pose_ref("orc", ordered, 0 if ordered else 250)
    n, hp = batch["n"], batch["hp"]
    ans = pose_answer(batch, want)
    rule = lambda *got: tc.check_pose_batch(case.scene, batch, want, got, ordered)
    assert max(rule(*ans)) < 1e-14                           # (the log of an identity, to rounding)
    b = 2                                                     # a frame of 120 observations, about 96 of them live
    assert want[b]["ran"] and int(hp[b, :n[b]].sum()) >= 20 and n[b] >= 40
    moved = lambda d: changed(ans, 0, (b, 9), lambda v: v + d)
    fails(rule, *moved(3e-8))                                                                           # a pose off by 3e-8
    if ordered:
        fails(rule, *moved(2e-10))
    else:
        # (inside the per-frame bound, but scale and errors are then only held to 1e-6: the looser branch is reached)
        tc.check_pose(n, hp, batch["T0"], want, *moved(1e-9))
    fails(rule, *changed(ans, 2, (b, 3), lambda v: v + 1))                                              # stats[3] off by one
    fails(rule, *changed(ans, 2, (b, 2), lambda v: v * (1 + 1e-8)))                                     # the final error, pose exact
    live = int(np.flatnonzero(ans[4][b, :n[b]])[0])
    fails(rule, *changed(ans, 4, (b, live), 0))                                                         # a pruning flag flipped
    fails(rule, *changed(ans, 1, (b, 7), lambda v: v * (1 + 1e-5) + 1e-13))                             # Cov
    fails(rule, *changed(ans, 3, b, 0))                                                                 # ran
    idle = next(i for i, o in enumerate(want) if not o["ran"])
    fails(rule, *changed(ans, 0, (idle, 9), lambda v: v + 1e-12))                                       # a frame that did not run is untouched
    beyond = next(i for i in range(len(n)) if n[i] < batch["ns"] and want[i]["ran"])
    flipped = changed(ans, 4, (beyond, batch["ns"] - 1), lambda v: 1 - v)
    tc.check_pose(n, hp, batch["T0"], want, *flipped, ordered=ordered)
    fails(tc.check_pose, n, hp, batch["T0"], want, *flipped, ordered=ordered, beyond_n=True)            # flags beyond n
    fails(tc.check_pose_median, [1e-11, 1e-11, 0.0])
    tc.check_pose_median([1e-9, 0.0, 0.0])


def test_pose_deferred_rule(case):
    batch = tc.pose_deferred_batch(case.scene)
    want = {n_iter: pose_answer(batch, tc.pose_want(case.checker("orc")[0], case.scene.cam, batch, n_iter)) for n_iter in (0, 10)}

    def run(n_iter, entry, leak=False):
        T, Cov, stats, ran, hp = (x.copy() for x in want[n_iter])
        if entry == "_deferred":   # the wave kernel alone: singular frames (and every frame at n_iter = 0) are handed over
            handed = (batch["n"] < 3) | (n_iter == 0)
            T[handed], hp[handed], ran[handed] = batch["T0"][handed], batch["hp"][handed], 2
            if leak:
                T[handed] += 1e-12
        return T, Cov, stats, ran, hp

    tc.check_pose_deferred(batch, run)
    fails(tc.check_pose_deferred, batch, lambda n_iter, entry: run(n_iter, entry, leak=True))


# ---- alignment, point optimizer, reprojection, selection, seed batches ------------------------------------------------------------
def test_alignment_rules(case):
    orc, pyrs, _, _ = case.checker("orc")
    M, n_iter = 96, 10
    tr = tc.align_trials(pyrs, np.random.default_rng(1), M, 2.5)
    ok, px, h = np.zeros(M, np.int32), np.zeros((M, 2)), np.zeros(M)
    for t in range(M):
        patch = tr["pwb"][t].reshape(10, 10)[1:9, 1:9].ravel()
        if tr["use_1d"][t]:
            ok[t], px[t], h[t] = orc.align1d(pyrs[tr["slot"][t]][tr["level"][t]], tr["dirs"][t], tr["pwb"][t], patch, n_iter, tr["px0"][t])
        else:
            ok[t], px[t] = orc.align2d(pyrs[tr["slot"][t]][tr["level"][t]], tr["pwb"][t], patch, n_iter, tr["px0"][t])
    ans = (ok, px, h)
    rule = lambda *a: tc.check_alignment(orc, pyrs, tr, n_iter, *a)
    assert rule(*ans) == ok.sum() > M // 4
    t2, t1 = int(np.flatnonzero((tr["use_1d"] == 0) & (ok == 1))[0]), int(np.flatnonzero((tr["use_1d"] == 1) & np.isfinite(h))[0])
    fails(rule, *changed(ans, 0, t2, 0))
    fails(rule, *changed(ans, 1, (t2, 0), lambda v: np.nextafter(v, 9e9)))
    fails(rule, *changed(ans, 2, t1, lambda v: np.nextafter(v, 9e9)))
    run = (px, ok, h, np.arange(M, dtype=np.int32))
    tc.same_alignment(run, tuple(x.copy() for x in run))
    tc.same_alignment(run, changed(run, 0, (M - 1, 0), lambda v: np.nextafter(v, 9e9)), M - 1)          # (beyond the compared head)
    for k, idx in ((0, (t2, 1)), (1, t2), (2, t1), (3, 5)):
        fails(tc.same_alignment, run, changed(run, k, idx, lambda v: np.nextafter(v, 9e9) if k in (0, 2) else v + 1))


def test_point_and_reprojection_rules(case):
    orc, scene = case.checker("orc")[0], case.scene
    ptr, fr, ff, p0 = tc.point_optimize_inputs(scene)
    out = p0.copy()
    for i in range(0, len(scene.obs), 3):
        out[i] = orc.point_optimize(np.array([scene.T_f_w[x[0]] for x in scene.obs[i]]), ff[ptr[i]:ptr[i + 1]], p0[i], 5)
    tc.check_point_optimize(orc, scene, ptr, ff, p0, out)
    fails(tc.check_point_optimize, orc, scene, ptr, ff, p0, changed((out,), 0, (3, 1), lambda v: v + 2e-11)[0])
    res = [orc.reproject_point(scene.cam, scene.T_f_w[scene.cur], p, 30, 22) for p in scene.pt_pos]
    ans = (np.array([r[0] for r in res], np.int32), np.array([r[1] for r in res]))
    tc.check_reproject_points(orc, scene, *ans)
    inside = int(np.flatnonzero(ans[0] >= 0)[0])
    fails(tc.check_reproject_points, orc, scene, *changed(ans, 0, inside, lambda v: v + 1))
    fails(tc.check_reproject_points, orc, scene, *changed(ans, 1, (inside, 0), lambda v: v + 2e-10))


def test_select_matches_rule(case):
    cam, rng = case.scene.cam, np.random.default_rng(7)
    trials = tc.select_trials(cam, rng, 300)
    sel, f, lvl, pos = pytrack.select_matches(cam, *trials, 40)
    ans = (len(sel), np.asarray(sel), np.asarray(f), np.asarray(lvl), np.asarray(pos), np.ones(len(sel), np.uint8))
    tc.check_select_matches(cam, trials, 40, *ans)
    fails(tc.check_select_matches, cam, trials, 40, len(sel) - 1, *ans[1:])
    for k, idx, d in ((1, 3, 1), (2, (3, 0), 2e-14), (3, 3, 1), (4, (3, 2), 1e-15)):   # sel, f, level, pos
        fails(tc.check_select_matches, cam, trials, 40, *changed(ans, k, idx, lambda v: v + d))
    fails(tc.check_select_matches, cam, trials, 40, *changed(ans, 5, 3, 0))                             # has_point


def test_seed_batch_rule(case):
    orc = case.checker("orc")[0]
    seeds, cols, x, tau2 = tc.seed_batch(orc, np.random.default_rng(9), 300)
    new = [orc.update_seed(x[i], tau2[i], seeds[i]) for i in range(len(seeds))]
    ans = dict(cols, **{k: np.array([getattr(s, k) for s in new], np.float32) for k in tc.STATE_KEYS})
    tc.check_seed_batch(orc, seeds, x, tau2, ans, min_identical=1.0)
    i = int(np.flatnonzero(np.isfinite([s.mu + s.sigma2 + s.a + s.b for s in new]))[5])
    for k, factor in (("mu", 1 + 4e-6), ("a", 1 + 2e-4), ("b", 1 + 2e-4), ("sigma2", 1 + 1e-2)):
        bad = dict(ans, **{k: ans[k].copy()})
        bad[k][i] *= np.float32(factor)
        fails(tc.check_seed_batch, orc, seeds, x, tau2, bad)
    bad = dict(ans, mu=ans["mu"].copy())
    bad["mu"][i] = np.nan
    fails(tc.check_seed_batch, orc, seeds, x, tau2, bad)


def test_frame_pose_model_is_a_rigid_product(case):
    """the host-side model of svo_hip_frame_pose_compose against se3.mul: the same product up to rounding"""
    rng = np.random.default_rng(2)
    for T, q, t in tc.frame_pose_compose_cases(rng, 40):
        w, x, y, z = q
        R = np.array([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                      2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)])
        want = se3.mul(T, np.concatenate([R, t]))
        assert np.abs(tc.host_frame_pose(T, q, t) - want).max() < 1e-12
