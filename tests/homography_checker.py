"""TEST INFRASTRUCTURE.  The f64 checker of svo_hip_homography_init (K9): the algorithm include/svo_hip.h states, restated
in numpy with its own linear algebra (numpy.linalg.svd for the decomposition, dense J'J for the refinement, literal
matrix products for the four-point homography) -- written from the header's text, not from the kernel.  One pair per
call.  Besides the outputs it reports how close every decision came to its threshold (`margins`), so that the case
builder can assert that no decision of a test case is a coin toss between two correct implementations."""
import numpy as np

OK, NO_MODEL, DEGENERATE = 0, 1, 2
FAILURE, SUCCESS = 0, 2
MASK = 0xFFFFFFFF


def fmix(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & MASK
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & MASK
    h ^= h >> 16
    return h


def draw(seed, k, m):
    """the four ranks of hypothesis k among m tracked points"""
    base = fmix((seed + 0x9E3779B9) & MASK)
    picks = []
    for j in range(4):
        h = fmix(base ^ ((4 * k + j) & MASK))
        r = (h * (m - j)) >> 32
        for p in sorted(picks):
            if r >= p:
                r += 1
        picks.append(r)
    return picks


def adjugate(M):
    """adj(M) for M [..., 3, 3]: its rows are the cross products of M's columns"""
    c = [M[..., :, i] for i in range(3)]
    return np.stack([np.cross(c[1], c[2]), np.cross(c[2], c[0]), np.cross(c[0], c[1])], axis=-2)


def four_point(P, Q):
    """P, Q [K, 4, 3] homogeneous points (draw order) -> (H [K, 3, 3], accepted [K])"""
    with np.errstate(all="ignore"):
        def frame(X):
            M = np.swapaxes(X[:, :3], 1, 2)                        # columns p1 p2 p3
            lam = np.einsum("kij,kj->ki", adjugate(M), X[:, 3])
            det = np.einsum("ki,ki->k", np.cross(X[:, 0], X[:, 1]), X[:, 2])
            q = (X * X).sum(axis=(1, 2))
            ok = (np.abs(det) >= 1e-10 * q) & (np.abs(lam) >= 1e-10 * q[:, None]).all(axis=1)
            return M * lam[:, None, :], ok                          # M diag(lambda)
        A, ok_a = frame(P)
        B, ok_b = frame(Q)
        G = B @ adjugate(A)
        H = G / G[:, 2:3, 2:3]
    return H, ok_a & ok_b & np.isfinite(H).all(axis=(1, 2))


def transfer_err2(H, uv_ref, uv_cur):
    """|uv_cur - project2d(H x_ref)|^2 per point; H [..., 3, 3]"""
    with np.errstate(all="ignore"):
        x = np.concatenate([uv_ref, np.ones((len(uv_ref), 1))], axis=1)
        y = np.einsum("...ij,nj->...ni", H, x)
        d = uv_cur - y[..., :2] / y[..., 2:3]
        return (d * d).sum(axis=-1)


def refine(H, uv_ref, uv_cur, iters):
    def evaluate(Hm):
        with np.errstate(all="ignore"):
            u, v = uv_ref[:, 0], uv_ref[:, 1]
            X, Y, W = (Hm[r, 0] * u + Hm[r, 1] * v + Hm[r, 2] for r in range(3))
            x, y = X / W, Y / W
            z, o = np.zeros_like(u), np.ones_like(u)
            Jx = np.stack([u, v, o, z, z, z, -x * u, -x * v], axis=1) / W[:, None]
            Jy = np.stack([z, z, z, u, v, o, -y * u, -y * v], axis=1) / W[:, None]
            J = np.concatenate([Jx, Jy])
            r = np.concatenate([uv_cur[:, 0] - x, uv_cur[:, 1] - y])
            return J.T @ J, J.T @ r, float(r @ r)

    def ldl_solve(A, b):
        with np.errstate(all="ignore"):
            n = len(b)
            L, d = np.eye(n), np.zeros(n)
            for j in range(n):
                d[j] = A[j, j] - (L[j, :j] ** 2 * d[:j]).sum()
                for i in range(j + 1, n):
                    L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j] * d[:j]).sum()) / d[j]
            y = np.zeros(n)
            for i in range(n):
                y[i] = b[i] - L[i, :i] @ y[:i]
            y = y / d
            x = np.zeros(n)
            for i in reversed(range(n)):
                x[i] = y[i] - L[i + 1:, i] @ x[i + 1:]
            return x

    if iters == 0:
        return H
    good, cost_good = H, None
    trial = H
    for it in range(iters + 1):
        A, b, cost = evaluate(trial)
        if it > 0 and not cost <= cost_good:
            break
        good, cost_good = trial, cost
        if it == iters:
            break
        delta = ldl_solve(A, b)
        if not np.isfinite(delta).all():
            break
        trial = (good.reshape(9) + np.append(delta, 0.0)).reshape(3, 3)
    return good


def decompose(H):
    """-> (list of 8 candidates dict(R, t, n, d), (d1, d2, d3)) or (None, d)"""
    with np.errstate(all="ignore"):
        U, d, Vt = np.linalg.svd(H)
        V = Vt.T
        for i in range(3):
            if V[np.argmax(np.abs(V[:, i])), i] < 0:
                V[:, i] = -V[:, i]
                U[:, i] = -U[:, i]
        if not (np.isfinite(U).all() and np.isfinite(V).all() and np.isfinite(d).all()):
            return None, d
        d1, d2, d3 = d
        if d1 - d2 < 1e-9 * d2 or d2 - d3 < 1e-9 * d2:
            return None, d
        s = -1.0 if np.linalg.det(U) * np.linalg.det(V) < 0 else 1.0
        x1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
        x3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        out = []
        for positive in (True, False):
            for e1, e3 in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
                if positive:
                    sn = (d1 - d3) * x1 * x3 * e1 * e3 / d2
                    cs = (d1 * x3 * x3 + d3 * x1 * x1) / d2
                    Rp = np.array([[cs, 0, -sn], [0, 1, 0], [sn, 0, cs]])
                    tp = (d1 - d3) * np.array([x1 * e1, 0, -x3 * e3])
                    dd = s * d2
                else:
                    sn = (d1 + d3) * x1 * x3 * e1 * e3 / d2
                    cs = (d3 * x1 * x1 - d1 * x3 * x3) / d2
                    Rp = np.array([[cs, 0, sn], [0, -1, 0], [sn, 0, -cs]])
                    tp = (d1 + d3) * np.array([x1 * e1, 0, x3 * e3])
                    dd = -s * d2
                out.append(dict(R=s * U @ Rp @ V.T, t=U @ tp, n=V @ np.array([x1 * e1, 0, x3 * e3]), d=dd))
        return out, d


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def sampson_sum(R, t, uv_ref, uv_cur, cap):
    with np.errstate(all="ignore"):
        E = skew(t) @ R
        x1 = np.concatenate([uv_ref, np.ones((len(uv_ref), 1))], axis=1)
        x2 = np.concatenate([uv_cur, np.ones((len(uv_cur), 1))], axis=1)
        Ex1, Etx2 = x1 @ E.T, x2 @ E
        e = (x2 * Ex1).sum(axis=1)
        err = e * e / (Ex1[:, 0] ** 2 + Ex1[:, 1] ** 2 + Etx2[:, 0] ** 2 + Etx2[:, 1] ** 2)
        terms = np.where(err < cap, err, cap)
        total = 0.0
        for v in terms:          # (the order differs from the device's: the sums agree to rounding)
            total += v
        return total


def closeness(value, threshold):
    """smallest relative distance of the finite values to the threshold"""
    value = np.asarray(value, np.float64).ravel()
    value = value[np.isfinite(value)]
    if value.size == 0:
        return np.inf
    return float(np.min(np.abs(value - threshold)) / abs(threshold))


def homography_init(cam, f_ref, f_cur, status, px_ref, px_cur, T_ref_w, reproj_thresh=2.0, min_inliers=40, map_scale=1.0,
                    n_hypotheses=512, refine_iters=10, seed=0):
    """One pair.  Returns a dict of every output of svo_hip_homography_out (numpy, the header's shapes and types) plus
    `margins` (dict: decision -> relative distance to its threshold), `gaps` ((d1 - d2) / d2, (d2 - d3) / d2) and
    `finalists` (the two (R, t) the choice ended with)."""
    n = len(status)
    out = dict(H=np.zeros(9), best_hypothesis=-1, n_inliers_H=0, inlier_H=np.zeros(n, np.uint8), T_cur_from_ref=np.zeros(12),
               ambiguous=0, status=NO_MODEL, xyz_in_cur=np.zeros((n, 3)), inlier=np.zeros(n, np.uint8), n_inliers=0,
               depth_median=0.0, scale=0.0, T_cur_w=np.zeros(12), point_w=np.zeros((n, 3)), point_ok=np.zeros(n, np.uint8),
               result=FAILURE, margins={}, gaps=None, finalists=None)
    idx = np.flatnonzero(np.asarray(status) != 0)
    m = len(idx)
    focal = abs(cam.fx)
    with np.errstate(all="ignore"):
        uv_ref = f_ref[idx, :2] / f_ref[idx, 2:3]
        uv_cur = f_cur[idx, :2] / f_cur[idx, 2:3]
    if m < 4:
        return out
    one = np.ones((m, 1))
    x_ref, x_cur = np.concatenate([uv_ref, one], axis=1), np.concatenate([uv_cur, one], axis=1)

    # 1. hypotheses
    picks = np.array([draw(seed, k, m) for k in range(n_hypotheses)])
    Hs, accepted = four_point(x_ref[picks], x_cur[picks])
    if not accepted.any():
        return out
    Hs[~accepted] = np.nan
    err2 = focal * focal * transfer_err2(Hs, uv_ref, uv_cur)              # [K, m]
    with np.errstate(all="ignore"):
        scores = np.where(accepted, (err2 < 4.0).sum(axis=1), -1)
    best = int(np.argmax(scores))                                           # (the first of the largest)
    out["margins"]["ransac"] = closeness(np.sqrt(err2[accepted]), 2.0)
    H = Hs[best]
    winners = err2[best] < 4.0

    # 2. refinement
    H = refine(H, uv_ref[winners], uv_cur[winners], refine_iters)

    # 3. inliers of H
    e_H = focal * np.sqrt(transfer_err2(H, uv_ref, uv_cur))
    with np.errstate(all="ignore"):
        in_H = e_H < reproj_thresh
    out["margins"]["inlier_H"] = closeness(e_H, reproj_thresh)
    out["H"], out["best_hypothesis"], out["n_inliers_H"] = H.reshape(9).copy(), best, int(in_H.sum())
    out["inlier_H"][idx] = in_H

    # 4. decomposition
    cands, d = decompose(H)
    if np.isfinite(d).all() and d[1] > 0:
        out["gaps"] = ((d[0] - d[1]) / d[1], (d[1] - d[2]) / d[1])
    if cands is None:
        out["status"] = DEGENERATE
        return out
    out["status"] = OK

    # 5. choice
    with np.errstate(all="ignore"):
        w = x_ref[in_H] @ H[2]
        score1 = [int((w / c["d"] > 0).sum()) for c in cands]
        order = sorted(range(8), key=lambda c: -score1[c])[:4]          # (sorted is stable)
        score2 = {c: int(((x_ref[in_H] @ cands[c]["n"]) / cands[c]["d"] > 0).sum()) for c in order}
        order = sorted(order, key=lambda c: -score2[c])[:2]
        first, second = cands[order[0]], cands[order[1]]
        ratio = np.float64(score2[order[1]]) / np.float64(score2[order[0]])
    out["margins"]["ratio"] = abs(float(ratio) - 0.9) / 0.9 if np.isfinite(ratio) else np.inf
    chosen = first
    if not ratio < 0.9:
        out["ambiguous"] = 1
        cap = 4.0 * (reproj_thresh / focal) ** 2
        s0 = sampson_sum(first["R"], first["t"], uv_ref, uv_cur, cap)
        s1 = sampson_sum(second["R"], second["t"], uv_ref, uv_cur, cap)
        out["margins"]["sampson"] = abs(s0 - s1) / max(abs(s0), abs(s1), 1e-300)
        if s1 < s0:
            chosen = second
    R, t = chosen["R"], chosen["t"]
    out["finalists"] = [(first["R"], first["t"]), (second["R"], second["t"])]
    out["T_cur_from_ref"] = np.concatenate([R.reshape(9), t])

    # 6. computeInliers
    with np.errstate(all="ignore"):
        fc, fr = f_cur[idx], f_ref[idx]
        f2 = fr @ R.T
        a00, a10, a11 = (fc * fc).sum(1), (fc * f2).sum(1), -(f2 * f2).sum(1)
        a01 = -a10
        b0, b1 = fc @ t, f2 @ t
        det = a00 * a11 - a01 * a10
        l0, l1 = (a11 * b0 - a01 * b1) / det, (a00 * b1 - a10 * b0) / det
        xyz = (l0[:, None] * fc + (t + l1[:, None] * f2)) / 2
        back = (xyz - t) @ R
        e1 = focal * np.linalg.norm(uv_cur - xyz[:, :2] / xyz[:, 2:3], axis=1)
        e2 = focal * np.linalg.norm(uv_ref - back[:, :2] / back[:, 2:3], axis=1)
        inl = (e1 <= reproj_thresh) & (e2 <= reproj_thresh)
    out["margins"]["inlier"] = min(closeness(e1, reproj_thresh), closeness(e2, reproj_thresh))
    out["inlier"][idx] = inl
    out["xyz_in_cur"][idx[inl]] = xyz[inl]
    out["n_inliers"] = int(inl.sum())
    if out["n_inliers"] < min_inliers or out["n_inliers"] == 0:
        return out

    # 7. scale and map
    z = np.sort(xyz[inl, 2], kind="stable")
    median = z[len(z) // 2]
    with np.errstate(all="ignore"):
        scale = map_scale / median
        R_rw, t_rw = T_ref_w[:9].reshape(3, 3), T_ref_w[9:]
        R_cw, t_cw = R @ R_rw, R @ t_rw + t
        pos_ref, pos_cur = -R_rw.T @ t_rw, -R_cw.T @ t_cw
        t_new = -R_cw @ (pos_ref + scale * (pos_cur - pos_ref))
        out["point_w"][idx[inl]] = (xyz[inl] * scale - t_new) @ R_cw
    out["depth_median"], out["scale"] = float(median), float(scale)
    out["T_cur_w"] = np.concatenate([R_cw.reshape(9), t_new])

    def in_frame(px):
        with np.errstate(all="ignore"):
            x, y = np.trunc(px[:, 0].astype(np.float64)), np.trunc(px[:, 1].astype(np.float64))
        return (x >= 10) & (x < cam.width - 10) & (y >= 10) & (y < cam.height - 10)
    ok = in_frame(px_cur[idx]) & in_frame(px_ref[idx]) & inl & (xyz[:, 2] > 0)
    out["point_ok"][idx] = ok
    out["result"] = SUCCESS
    return out
