"""Independent numpy re-derivations of the third-party arithmetic the oracle restates from published
sources (rpg_vikit, fast, boost::math, Sophus, Eigen are un-vendored and un-pinned): the depth-filter
closed forms, the FAST-10 detector with its score / non-max rules, vk::shiTomasiScore, Sophus SE3::exp against the matrix
exponential, and the two optimisers built on those pieces end to end -- pose_optimizer::optimizeGaussNewton (robust cost,
median, LDLT, exp) and SparseImgAlign::run on vk::NLLSSolver's Gauss-Newton loop -- each in float64 from the published
algorithm, not from the restatement.  CPU only."""
import math

import numpy as np

from oracle import pytrack


def test_update_seed_matches_float64_derivation(oracle):
    """Vogiatzis & Hernandez moment matching (depth_filter.cpp:309-332) re-derived in float64."""
    orc = pytrack.Track("orc")
    rng = np.random.default_rng(0)
    for _ in range(200):
        s = orc.seed_init(rng.uniform(0.5, 5.0), rng.uniform(0.2, 0.45))
        s.a, s.b = np.float32(rng.uniform(5, 40)), np.float32(rng.uniform(5, 40))
        s.mu = np.float32(s.mu * rng.uniform(0.8, 1.2))
        x = float(s.mu) * rng.uniform(0.9, 1.1)
        tau2 = (float(s.mu) * rng.uniform(0.005, 0.05)) ** 2
        a, b, mu, s2, zr = float(s.a), float(s.b), float(s.mu), float(s.sigma2), float(s.z_range)
        norm_scale = math.sqrt(s2 + tau2)
        pdf = math.exp(-0.5 * ((x - mu) / norm_scale) ** 2) / (norm_scale * math.sqrt(2 * math.pi))
        ss2 = 1.0 / (1.0 / s2 + 1.0 / tau2)
        m = ss2 * (mu / s2 + x / tau2)
        C1, C2 = a / (a + b) * pdf, b / (a + b) / zr
        C1, C2 = C1 / (C1 + C2), C2 / (C1 + C2)
        f = C1 * (a + 1) / (a + b + 1) + C2 * a / (a + b + 1)
        e = C1 * (a + 1) * (a + 2) / ((a + b + 1) * (a + b + 2)) + C2 * a * (a + 1) / ((a + b + 1) * (a + b + 2))
        mu_new = C1 * m + C2 * mu
        s2_new = C1 * (ss2 + m * m) + C2 * (s2 + mu * mu) - mu_new * mu_new
        a_new = (e - f) / (f - e / f)
        b_new = a_new * (1 - f) / f
        o = orc.update_seed(x, tau2, s)
        assert np.isclose(o.mu, mu_new, rtol=2e-5)
        assert abs(o.sigma2 - s2_new) <= 2e-3 * s2_new + 1e-6 * mu * mu      # float cancellation in the reference
        assert np.isclose(o.a, a_new, rtol=5e-2) and np.isclose(o.b, b_new, rtol=5e-2)


def test_compute_tau_is_the_law_of_sines(oracle):
    """depth_filter.cpp:334-350 with the reference's PI = 3.14159265 (global.h:78)."""
    orc = pytrack.Track("orc")
    rng = np.random.default_rng(1)
    for _ in range(100):
        t = rng.normal(size=3) * 0.2
        f = rng.normal(size=3); f[2] = abs(f[2]) + 1.0; f /= np.linalg.norm(f)
        z = rng.uniform(0.5, 5.0)
        ang = 2 * math.atan(1.0 / (2 * 315.5))
        T = np.concatenate([np.eye(3).reshape(9), t])
        a = f * z - t
        alpha = math.acos(f @ t / np.linalg.norm(t))
        beta = math.acos(a @ (-t) / (np.linalg.norm(t) * np.linalg.norm(a)))
        gamma_plus = 3.14159265 - alpha - (beta + ang)
        z_plus = np.linalg.norm(t) * math.sin(beta + ang) / math.sin(gamma_plus)
        assert np.isclose(orc.compute_tau(T, f, z, ang), z_plus - z, rtol=1e-10, atol=1e-14)


def test_fast10_score_nonmax_and_shi_tomasi_against_brute_force(oracle):
    """(the brute force lives in tests/fast_reference.py, which extends it to the whole of FastDetector::detect)"""
    import fast_reference as fr
    rng = np.random.default_rng(3)
    h, w = 40, 56
    img = rng.integers(0, 256, size=(h, w)).astype(np.uint8)
    img[10:30, 12:40] = (img[10:30, 12:40] // 4 + 150).astype(np.uint8)   # a brighter block: real corners and edges
    pyr = oracle.create_img_pyramid(img, 1)
    # cell size 1: every pixel is its own grid cell, so the grid output IS the list of surviving corners
    xy, lvl, sc, n = pytrack.fast_detect_grid(pyr, 1, 1, w, h, None, 20, 0.0)
    got = {(int(x), int(y)): float(s) for (x, y), s, l in zip(xy, sc, lvl) if l >= 0}
    S = fr.fast_scores(img, 20)   # fast_corner_score_10: largest threshold that still passes, -1 where no corner
    corners = {(int(x), int(y)): int(S[y, x]) for y, x in zip(*np.nonzero(S >= 0))}
    assert len(corners) > 30
    assert all(3 <= x < w - 3 and 3 <= y < h - 3 and fr.is_corner(img, x, y, s) and not fr.is_corner(img, x, y, s + 1) for (x, y), s in corners.items())
    expect = {}
    keep = fr.nonmax_3x3(S)       # fast_nonmax_3x3: a neighbouring corner with score >= own suppresses
    for (x, y), s in corners.items():
        if not keep[y, x]:
            continue
        lam = fr.shi_tomasi(img, x, y)   # vk::shiTomasiScore returns 0 next to the border: never above the threshold
        if lam > 0.0:
            expect[(x, y)] = lam
    assert set(got) == set(expect)
    for k, v in expect.items():
        assert np.isclose(got[k], v, rtol=1e-4), (k, got[k], v)


def _expm_se3(xi):
    """exp of the twist (upsilon, omega) as a 4x4 matrix exponential (scipy): what Sophus SE3::exp computes in closed form"""
    from scipy.linalg import expm
    u, w = xi[:3], xi[3:]
    M = np.zeros((4, 4))
    M[:3, :3] = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    M[:3, 3] = u
    return expm(M)


def test_se3_exp_is_the_matrix_exponential(oracle):
    """The oracle's restatement of Sophus SE3::exp (closed form: Rodrigues + V(omega) upsilon) against scipy's Pade matrix
    exponential of the 4x4 twist, over small and large rotations."""
    from oracle import pyoracle
    rng = np.random.default_rng(5)
    for scale in (1e-9, 1e-5, 1e-2, 0.5, 2.5):
        for _ in range(20):
            xi = rng.normal(size=6) * scale
            T = np.asarray(pyoracle.se3_exp(xi))
            E = _expm_se3(xi)
            assert np.allclose(T[:9].reshape(3, 3), E[:3, :3], rtol=0, atol=5e-13), (scale, xi)
            assert np.allclose(T[9:], E[:3, 3], rtol=1e-12, atol=5e-13), (scale, xi)


def _pose_optimize_numpy(fx, T_f_w, f, level, has_point, pos, reproj_thresh, n_iter):
    """pose_optimizer::optimizeGaussNewton (svo/src/pose_optimizer.cpp:28-161) re-derived in numpy float64 from the published
    pieces it is built of: vk::project2d, Frame::jacobian_xyz2uv (frame.h:116-138), vk::robust_cost::TukeyWeightFunction
    (b = 4.6851, a FLOAT function of a float argument), MADScaleEstimator (1.48 x median, on FLOAT errors as the reference
    stores them), vk::getMedian (the element
    at n / 2 of the sorted values), a dense solve for A.ldlt().solve(b), and the matrix exponential for SE3::exp."""
    R, t = np.array(T_f_w[:9]).reshape(3, 3), np.array(T_f_w[9:])
    idx = [i for i in range(len(f)) if has_point[i]]
    if not idx:
        return None
    proj = lambda v: v[:2] / v[2]
    inv_cov = lambda i: 1.0 / (1 << int(level[i]))
    med = lambda v: sorted(v)[len(v) // 2]

    def errors(R, t):
        return [(proj(f[i]) - proj(R @ pos[i] + t)) * inv_cov(i) for i in idx]

    e32 = [np.float32(np.linalg.norm(e)) for e in errors(R, t)]
    est_scale = float(np.float32(1.48) * med(e32))
    scale, chi2 = est_scale, 0.0
    R_old, t_old = R.copy(), t.copy()
    chi2_init = None
    A = np.zeros((6, 6))
    for it in range(n_iter):
        if it == 5:
            scale = 0.85 / fx
        A, b, new_chi2 = np.zeros((6, 6)), np.zeros(6), 0.0
        sq = []
        for i in idx:
            x, y, z = R @ pos[i] + t
            zi = 1.0 / z
            J = np.array([[-zi, 0, x * zi * zi, x * y * zi * zi, -(1 + x * x * zi * zi), y * zi],
                          [0, -zi, y * zi * zi, 1 + y * y * zi * zi, -x * y * zi * zi, -x * zi]]) * inv_cov(i)
            e = (proj(f[i]) - np.array([x * zi, y * zi])) * inv_cov(i)
            sq.append(e @ e)
            # vikit's weight functions are float: value(const float& x), b = 4.6851f, b * b and the result in float
            r = np.float32(np.linalg.norm(e) / scale)
            r2, b2 = r * r, np.float32(4.6851) * np.float32(4.6851)
            w = float((np.float32(1.0) - r2 / b2) ** 2) if r2 <= b2 else 0.0
            A += J.T @ J * w
            b -= J.T @ e * w
            new_chi2 += (e @ e) * w
        if it == 0:
            chi2_init = sq
        dT = np.linalg.solve(A, b)
        if (it > 0 and new_chi2 > chi2) or np.isnan(dT[0]):
            R, t = R_old, t_old
            break
        E = _expm_se3(dT)
        R_old, t_old = R, t
        R, t = E[:3, :3] @ R, E[:3, :3] @ t + E[:3, 3]
        chi2 = new_chi2
        if np.abs(dT).max() <= 1e-10:
            break
    final = [e @ e for e in errors(R, t)]
    thresh = reproj_thresh / fx
    hp = np.array(has_point, dtype=np.uint8).copy()
    for k, i in enumerate(idx):
        if np.sqrt(final[k]) > thresh:
            hp[i] = 0
    return dict(T=np.concatenate([R.ravel(), t]), has_point=hp, num_obs=int(hp[idx].sum()),
                estimated_scale=est_scale * fx, error_init=np.sqrt(med(chi2_init)) * fx, error_final=np.sqrt(med(final)) * fx,
                Cov=np.linalg.inv(A * fx * fx))


def test_pose_optimizer_against_a_numpy_derivation(oracle):
    """The oracle's optimizeGaussNewton -- with its restated Eigen LDLT, Sophus exp, vikit robust cost and median -- against
    the derivation above on tracked frames with outliers: pose to 1e-9 (SE(3) log-norm), the same observations pruned, the
    reported scale / errors / covariance."""
    from helpers import camera_models
    from rpg_svo_amd import se3, synth
    orc = pytrack.Track("orc")
    scene = synth.make_track_scene(n_kf=3, n_feat=120, cam=camera_models()["pinhole"])
    rng = np.random.default_rng(8)
    P = len(scene.pt_pos)
    for trial in range(6):
        f = synth._bearing(scene.cam, scene.px_true + rng.normal(size=(P, 2)) * 0.4)
        level = rng.integers(0, 3, size=P).astype(np.int32)
        pos = scene.pt_pos.copy()
        bad = rng.choice(P, size=P // 12, replace=False)
        pos[bad] += rng.normal(size=(len(bad), 3)) * 0.15                  # outliers the Tukey weight and the pruning meet
        hp = (rng.uniform(size=P) > 0.15).astype(np.uint8)
        T0 = se3.mul(se3.exp(rng.normal(size=6) * 4e-3), scene.T_f_w[scene.cur])
        o = orc.pose_optimize(scene.cam, T0, f, level, hp, pos, 2.0, 10)
        n = _pose_optimize_numpy(scene.cam.fx, T0, f, level, hp, pos, 2.0, 10)
        assert o["ran"] and n is not None
        assert se3.log_norm(o["T_f_w"][None], n["T"][None])[0] < 1e-9, trial
        assert np.array_equal(o["has_point"], n["has_point"]) and o["num_obs"] == n["num_obs"]
        assert 0 < n["num_obs"] < int(hp.sum())                           # something was pruned, not everything
        assert np.isclose(o["estimated_scale"], n["estimated_scale"], rtol=1e-6)      # (a float product in the reference)
        assert np.isclose(o["error_init"], n["error_init"], rtol=1e-9) and np.isclose(o["error_final"], n["error_final"], rtol=1e-7)
        assert np.allclose(o["Cov"], n["Cov"], rtol=1e-6, atol=1e-16)


def _sparse_img_align_numpy(ref_pyr, cur_pyr, cam, T_ref_w, T_cur_w, px, f, pos, max_level, min_level, n_iter=30, eps=1e-6):
    """SparseImgAlign::run (svo/src/sparse_img_align.cpp:43-258) on top of vk::NLLSSolver::optimizeGaussNewton (rpg_vikit
    nlls_solver_impl.hpp), re-derived in numpy FLOAT64 from the published algorithm: inverse-compositional photometric
    alignment of 4x4 patches, reference Jacobians cached per level, Gauss-Newton with roll-back when the mean squared
    residual rises, T <- T exp(-x).  Not a restatement of the reference's float arithmetic: agreement is to the f32 noise of
    the reference's pixels, and the iteration counts may differ where a chi2 comparison sits on that noise."""
    def split(T):
        return np.array(T[:9]).reshape(3, 3), np.array(T[9:])
    Rr, tr = split(T_ref_w)
    Rc, tc = split(T_cur_w)
    R, t = Rc @ Rr.T, tc - Rc @ Rr.T @ tr                                   # T_cur_from_ref = T_cur_w * T_ref_w^-1
    ref_pos = -Rr.T @ tr
    depth = np.linalg.norm(pos - ref_pos, axis=1)
    xyz_ref = f * depth[:, None]
    offs = np.arange(4) - 2
    iters = []

    def sample(img, u, v):                                                  # bilinear, u / v arrays of the same shape
        ui, vi = np.floor(u).astype(int), np.floor(v).astype(int)
        su, sv = u - ui, v - vi
        I = img.astype(np.float64)
        return ((1 - su) * (1 - sv) * I[vi, ui] + su * (1 - sv) * I[vi, ui + 1] + (1 - su) * sv * I[vi + 1, ui] + su * sv * I[vi + 1, ui + 1])

    visible = np.zeros(len(px), bool)                                       # (never reset between levels, as in the reference)
    for level in range(max_level, min_level - 1, -1):
        ref_img, cur_img = ref_pyr[level], cur_pyr[level]
        h, w = ref_img.shape
        scale = 1.0 / (1 << level)
        u_ref, v_ref = px[:, 0] * scale, px[:, 1] * scale
        ui, vi = np.floor(u_ref).astype(int), np.floor(v_ref).astype(int)
        visible |= (ui - 3 >= 0) & (vi - 3 >= 0) & (ui + 3 < w) & (vi + 3 < h)
        idx = np.nonzero(visible)[0]
        # reference patches and their Jacobians (:107-141): I, dx, dy at the 16 pixels around the sub-pixel position
        gu = u_ref[idx, None, None] + offs[None, None, :]                   # [n, y, x]
        gv = v_ref[idx, None, None] + offs[None, :, None]
        gu, gv = np.broadcast_arrays(gu, gv)
        I_ref = sample(ref_img, gu, gv)
        dx = 0.5 * (sample(ref_img, gu + 1, gv) - sample(ref_img, gu - 1, gv))
        dy = 0.5 * (sample(ref_img, gu, gv + 1) - sample(ref_img, gu, gv - 1))
        x, y, z = xyz_ref[idx, 0], xyz_ref[idx, 1], xyz_ref[idx, 2]
        zi = 1.0 / z
        J0 = np.stack([-zi, 0 * zi, x * zi * zi, x * y * zi * zi, -(1 + x * x * zi * zi), y * zi], -1)       # frame.h:116-138
        J1 = np.stack([0 * zi, -zi, y * zi * zi, 1 + y * y * zi * zi, -x * y * zi * zi, -x * zi], -1)
        Jc = (dx[..., None] * J0[:, None, None, :] + dy[..., None] * J1[:, None, None, :]) * (cam.fx / (1 << level))
        chi2, n_eval = 0.0, 0
        R_old, t_old = R, t
        for it in range(n_iter):
            p = xyz_ref[idx] @ R.T + t
            uc = (cam.fx * p[:, 0] / p[:, 2] + cam.cx) * scale
            vc = (cam.fy * p[:, 1] / p[:, 2] + cam.cy) * scale
            uci, vci = np.floor(uc).astype(int), np.floor(vc).astype(int)
            ok = (uci - 3 >= 0) & (vci - 3 >= 0) & (uci + 3 < w) & (vci + 3 < h)
            cu = uc[ok, None, None] + offs[None, None, :]
            cv = vc[ok, None, None] + offs[None, :, None]
            cu, cv = np.broadcast_arrays(cu, cv)
            res = sample(cur_img, cu, cv) - I_ref[ok]
            n_eval += 1
            Jv = Jc[ok].reshape(-1, 6)
            rv = res.reshape(-1)
            H, Jres = Jv.T @ Jv, -Jv.T @ rv
            new_chi2 = float(rv @ rv) / max(len(rv), 1)
            try:
                xs = np.linalg.solve(H, Jres)
            except np.linalg.LinAlgError:
                xs = np.full(6, np.nan)
            if (it > 0 and new_chi2 > chi2) or np.isnan(xs[0]):
                R, t = R_old, t_old                                         # roll back and leave the level
                break
            E = _expm_se3(-xs)
            R_old, t_old = R, t
            R, t = R @ E[:3, :3], R @ E[:3, 3] + t                          # T <- T exp(-x)
            chi2 = new_chi2
            if np.abs(xs).max() <= eps:
                break
        iters.append(n_eval)
    Rn, tn = R @ Rr, R @ tr + t                                              # cur.T_f_w = T_cur_from_ref * ref.T_f_w
    return np.concatenate([Rn.ravel(), tn]), iters


def test_sparse_img_align_against_a_numpy_derivation(oracle):
    """The oracle's SparseImgAlign::run -- restated vikit NLLSSolver loop, Sophus, Eigen LDLT, f32 pixel arithmetic -- against
    the float64 derivation above on rendered frame pairs, coarse to fine over all four levels: the refined pose to 2e-6
    (SE(3) log-norm; measured 0.7e-7 .. 1.4e-7: the reference's own f32 pixel noise), both within 1e-3 of the ground truth the
    prior was 1e-2 away from, and the same number of residual evaluations per level (measured: all 20 identical)."""
    from helpers import make_batch
    from rpg_svo_amd import se3, synth
    seq = synth.make_sequence(6, 120)
    pairs = [(i, i + 1) for i in range(5)]
    b = make_batch(seq, pairs, 4)
    same_iters, total = 0, 0
    for k, (r, c) in enumerate(pairs):
        ref_pyr = oracle.create_img_pyramid(b.images[r], 4)
        cur_pyr = oracle.create_img_pyramid(b.images[c], 4)
        T_o, res = oracle.sparse_img_align_run(ref_pyr, cur_pyr, b.cam, b.T_ref_w[k], b.T_cur_w[k], b.px[k], b.f[k], b.has_point[k],
                                               b.pos[k], 3, 0)
        T_n, iters = _sparse_img_align_numpy(ref_pyr, cur_pyr, b.cam, b.T_ref_w[k], b.T_cur_w[k], b.px[k], b.f[k], b.pos[k], 3, 0)
        d = se3.log_norm(T_o[None], T_n[None])[0]
        assert d < 2e-6, (k, d)
        assert se3.log_norm(T_n[None], b.T_gt_w[k][None])[0] < 1e-3 and se3.log_norm(T_o[None], b.T_gt_w[k][None])[0] < 1e-3
        assert se3.log_norm(b.T_cur_w[k][None], b.T_gt_w[k][None])[0] > 3e-3     # (the prior was far: something was optimised)
        o_iters = [int(res["iters"][lv]) for lv in (3, 2, 1, 0)]
        same_iters += sum(a == bb for a, bb in zip(o_iters, iters))
        total += 4
    assert same_iters >= total * 0.9, (same_iters, total)
