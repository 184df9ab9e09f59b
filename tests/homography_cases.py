"""TEST INFRASTRUCTURE.  The cases of the homography tests (numpy only): synthetic two-view geometry with its ground truth,
the batches the emulated and the GPU tests run, the checker's answer for every pair (computed once per process), and the
comparison rule.

Geometry: points of a plane at depth 2 in the reference view whose normal is tilted by at most 0.1, with or without 3 %
relief; a rotation of at most 2 degrees and a baseline of 0.4 (at most half of it along the optical axis, so every depth
stays above 0.5 in both views -- scenes with points behind a camera are not physical and not used); a 752 x 480 pinhole
camera with focal length 315.5.  Pixel noise 0 or 0.3 px, outliers 0 or 30 % (uniform +-30 px).  Bearings are formed from
the f64 pixel positions, px_ref / px_cur are their f32 roundings (the entry uses them for the 10 px border rule only).
Lost points are interleaved with the tracked ones and carry NaN bearings: nothing of theirs may be read.

Comparison rule (compare): every discrete output equals the checker's on every pair and point.  Nothing is exempt: the
builder asserts that no decision of any case lies within 1e-9 relative of its threshold in the checker (`margins`).
Continuous outputs are compared on the pairs whose singular-value gaps are at least 1e-3 in the checker."""
import functools
import types

import numpy as np

import homography_checker as chk

DISCRETE = ("best_hypothesis", "n_inliers_H", "inlier_H", "ambiguous", "status", "inlier", "n_inliers", "point_ok", "result")
CONTINUOUS = ("H", "T_cur_from_ref", "xyz_in_cur", "depth_median", "scale", "T_cur_w", "point_w")
MARGIN = 1e-9
MIN_GAP = 1e-3
DEFAULTS = dict(reproj_thresh=2.0, min_inliers=40, map_scale=1.0, n_hypotheses=512, refine_iters=10, seed=0)


def camera():
    return types.SimpleNamespace(width=752, height=480, fx=315.5, fy=315.5, cx=376.0, cy=240.0, model=0, d=(0.0,) * 5)


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def rotation_angle(Ra, Rb):
    D = Ra.T @ Rb                      # (atan2 of sine and cosine: arccos alone cannot resolve angles below 1e-8)
    sine = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(sine, (np.trace(D) - 1) / 2))


def direction_angle(a, b):
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), np.dot(a, b)))


def make_pair(seed, m, noise=0.3, outliers=0.3, relief=0.03, n_lost=None, identity_pose=False, identical_views=False):
    """m tracked points and n_lost lost ones (default m // 3, interleaved; capped so that n_pts <= 1024)"""
    rng = np.random.default_rng(seed)
    cam = camera()
    n_lost = min(m // 3 if n_lost is None else n_lost, 1024 - m)
    n = m + n_lost
    status = np.ones(n, np.uint8)
    if n_lost:
        status[np.linspace(0, n - 1, n_lost + 2)[1:-1].astype(int)] = 0
        extra = n_lost - int((status == 0).sum())            # (linspace may repeat an index on tiny cases)
        free = np.flatnonzero(status)
        status[free[:extra]] = 0
    idx = np.flatnonzero(status)
    assert len(idx) == m
    px_r = np.stack([rng.uniform(12, cam.width - 12, m), rng.uniform(12, cam.height - 12, m)], axis=1)
    ray = np.stack([(px_r[:, 0] - cam.cx) / cam.fx, (px_r[:, 1] - cam.cy) / cam.fy, np.ones(m)], axis=1)
    normal = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), 1.0])
    normal /= np.linalg.norm(normal)
    depth = 2.0 * normal[2] / (ray @ normal)                   # the plane through (0, 0, 2)
    depth = depth * (1 + relief * rng.uniform(-1, 1, m))
    X_ref = ray * depth[:, None]
    axis = rng.normal(size=3)
    R = rodrigues(axis / np.linalg.norm(axis) * np.deg2rad(rng.uniform(0.5, 2.0)))
    tdir = rng.normal(size=3)
    tdir[2] = np.clip(tdir[2], -0.5, 0.5) * np.linalg.norm(tdir[:2])
    t = 0.4 * tdir / np.linalg.norm(tdir)
    if identical_views:
        R, t = np.eye(3), np.zeros(3)
    X_cur = X_ref @ R.T + t
    assert X_ref[:, 2].min() > 0.5 and X_cur[:, 2].min() > 0.5
    px_c = np.stack([cam.fx * X_cur[:, 0] / X_cur[:, 2] + cam.cx, cam.fy * X_cur[:, 1] / X_cur[:, 2] + cam.cy], axis=1)
    good = np.ones(m, bool)
    if noise:
        px_r = px_r + rng.normal(0, noise, px_r.shape)
        px_c = px_c + rng.normal(0, noise, px_c.shape)
    if outliers:
        bad = rng.permutation(m)[:int(round(outliers * m))]
        px_c[bad] += rng.uniform(-30, 30, (len(bad), 2))
        good[bad] = False

    def bearing(px):
        f = np.stack([(px[:, 0] - cam.cx) / cam.fx, (px[:, 1] - cam.cy) / cam.fy, np.ones(len(px))], axis=1)
        return f / np.linalg.norm(f, axis=1, keepdims=True)
    p = types.SimpleNamespace(cam=cam, n_pts=n, m=m, seed=seed)
    p.status = status
    p.f_ref, p.f_cur = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
    p.f_ref[idx], p.f_cur[idx] = bearing(px_r), bearing(px_c)
    p.px_ref, p.px_cur = np.full((n, 2), -777.0, np.float32), np.full((n, 2), -777.0, np.float32)
    p.px_ref[idx], p.px_cur[idx] = px_r.astype(np.float32), px_c.astype(np.float32)
    if identity_pose:
        p.T_ref_w = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    else:
        aw = rng.normal(size=3)
        p.T_ref_w = np.concatenate([rodrigues(aw / np.linalg.norm(aw) * 0.3).reshape(9), rng.uniform(-1, 1, 3)])
    p.truth = types.SimpleNamespace(R=R, t=t, X_ref=np.zeros((n, 3)), good=np.zeros(n, bool))
    p.truth.X_ref[idx], p.truth.good[idx] = X_ref, good
    return p


def collinear_pair(seed, m=60):
    """every tracked point on one line of the unit plane in both views: each hypothesis has three collinear points"""
    p = make_pair(seed, m, noise=0.0, outliers=0.0, relief=0.0, n_lost=5)
    idx = np.flatnonzero(p.status)
    s = np.linspace(-0.9, 0.9, m)
    for f, (a, b, c, d) in ((p.f_ref, (0.5, 0.1, 0.25, -0.05)), (p.f_cur, (0.48, 0.15, 0.26, -0.02))):
        x = np.stack([a * s + b, c * s + d, np.ones(m)], axis=1)
        f[idx] = x / np.linalg.norm(x, axis=1, keepdims=True)
    return p


def poisoned_pair(seed, m=120):
    """NaN and infinite bearings on a few tracked points"""
    p = make_pair(seed, m, noise=0.3, outliers=0.0, relief=0.03)
    idx = np.flatnonzero(p.status)
    p.f_ref[idx[3]] = np.nan
    p.f_cur[idx[17], 0] = np.inf
    p.f_cur[idx[40], 2] = 0.0          # uv = +-inf
    p.f_ref[idx[77], 1] = -np.inf
    p.f_cur[idx[99]] = np.nan
    p.truth.good[idx[[3, 17, 40, 77, 99]]] = False
    return p


def border_pair(seed, m=100):
    """px_ref / px_cur of the first points at the exact limits of isInFrame(int(px), 10): 9.99 is out (int 9), 10.0 in,
    width - 10 - 0.01 in (int width - 11), width - 10 out; likewise in y; every combination of view and axis"""
    p = make_pair(seed, m, noise=0.0, outliers=0.0, relief=0.03, n_lost=7)
    idx = np.flatnonzero(p.status)
    w, h = p.cam.width, p.cam.height
    xs = [9.99, 10.0, w - 10 - 0.01, w - 10.0]
    ys = [9.99, 10.0, h - 10 - 0.01, h - 10.0]
    k = 0
    for arr in (p.px_ref, p.px_cur):
        other = p.px_cur if arr is p.px_ref else p.px_ref
        for axis, vals in ((0, xs), (1, ys)):
            for v in vals:
                arr[idx[k]] = (200.0, 200.0)
                other[idx[k]] = (300.0, 100.0)
                arr[idx[k], axis] = v
                k += 1
    p.n_border = k
    return p


def _batch(name, pairs, **params):
    assert len({p.n_pts for p in pairs}) == 1
    return types.SimpleNamespace(name=name, pairs=pairs, params={**DEFAULTS, **params}, n_pts=pairs[0].n_pts, cam=pairs[0].cam)


@functools.lru_cache(maxsize=None)
def batches():
    """name -> batch.  (Built once per process; the arrays are never written by the tests.)"""
    out = []
    # point counts around the strides of the kernel's loops (64 lanes, 256 work-items, 1024 points), one pair each
    for m in (4, 5):
        out.append(_batch(f"m{m}", [make_pair(100 + m, m, noise=0.0, outliers=0.0, relief=0.0, n_lost=1)], min_inliers=4))
    for m in (63, 64, 65, 255, 256, 257, 352):
        out.append(_batch(f"m{m}", [make_pair((1064 if m == 64 else 100 + m), m)]))   # (seed 164 has a score ratio of exactly 0.9)
    out.append(_batch("m1024", [make_pair(1124, 1024)]))
    out.append(_batch("m768of1024", [make_pair(868, 768, n_lost=256)]))
    # batches: identical pairs at different positions, failed pairs between good ones
    a, b = make_pair(11, 90, n_lost=30), make_pair(12, 90, n_lost=30)
    out.append(_batch("three_pairs", [a, b, a], n_hypotheses=64))
    c = make_pair(13, 90, noise=0.0, outliers=0.0, relief=0.0, n_lost=30)
    none, three = make_pair(14, 90, n_lost=30), make_pair(15, 90, n_lost=30)
    none.status = np.zeros_like(none.status)
    three.status = three.status.copy()
    three.status[np.flatnonzero(three.status)[3:]] = 0
    out.append(_batch("five_pairs", [c, none, a, three, c], n_hypotheses=64))
    # parameters away from their defaults
    out.append(_batch("one_hypothesis", [make_pair(21, 100)], n_hypotheses=1))
    out.append(_batch("no_refinement", [make_pair(22, 100)], refine_iters=0))
    out.append(_batch("tight_threshold", [make_pair(23, 100)], reproj_thresh=1.0))
    out.append(_batch("too_few_inliers", [make_pair(24, 100)], min_inliers=200))
    out.append(_batch("map_scale_seed", [make_pair(25, 100)], map_scale=2.5, seed=7, min_inliers=10))
    # degenerate inputs
    out.append(_batch("four_tracked", [make_pair(31, 4, noise=0.0, outliers=0.0, relief=0.0, n_lost=60)], min_inliers=4))
    out.append(_batch("collinear", [collinear_pair(32)]))
    out.append(_batch("identical_views", [make_pair(33, 80, noise=0.0, outliers=0.0, relief=0.0, identical_views=True)]))
    out.append(_batch("nan_inf_bearings", [poisoned_pair(34)]))
    out.append(_batch("border", [border_pair(35)]))
    out = {b.name: b for b in out}
    for b in out.values():
        for p in b.pairs:
            if not hasattr(p, "expect") or p.expect_params != b.params:
                p.expect = chk.homography_init(p.cam, p.f_ref, p.f_cur, p.status, p.px_ref, p.px_cur, p.T_ref_w, **b.params)
                p.expect_params = b.params
            close = {k: v for k, v in p.expect["margins"].items() if v < MARGIN}
            assert not close, f"{b.name}: the checker puts a decision within {MARGIN} of its threshold: {close}"
        b.expect = [p.expect for p in b.pairs]
    return out


NAMES = ("m4", "m5", "m63", "m64", "m65", "m255", "m256", "m257", "m352", "m1024", "m768of1024", "three_pairs", "five_pairs",
         "one_hypothesis", "no_refinement", "tight_threshold", "too_few_inliers", "map_scale_seed", "four_tracked", "collinear",
         "identical_views", "nan_inf_bearings", "border")


def inputs(b):
    """the arrays of a batch as the entry takes them"""
    st = lambda k, dt: np.ascontiguousarray(np.stack([getattr(p, k) for p in b.pairs]), dtype=dt)
    return dict(f_ref=st("f_ref", np.float64), f_cur=st("f_cur", np.float64), status=st("status", np.uint8),
                px_ref=st("px_ref", np.float32), px_cur=st("px_cur", np.float32), T_ref_w=st("T_ref_w", np.float64))


def out_shapes(n_pairs, n_pts):
    """name -> (shape, dtype) of svo_hip_homography_out, in the struct's order"""
    return dict(H=((n_pairs, 9), np.float64), best_hypothesis=((n_pairs,), np.int32), n_inliers_H=((n_pairs,), np.int32),
                inlier_H=((n_pairs, n_pts), np.uint8), T_cur_from_ref=((n_pairs, 12), np.float64), ambiguous=((n_pairs,), np.int32),
                status=((n_pairs,), np.int32), xyz_in_cur=((n_pairs, n_pts, 3), np.float64), inlier=((n_pairs, n_pts), np.uint8),
                n_inliers=((n_pairs,), np.int32), depth_median=((n_pairs,), np.float64), scale=((n_pairs,), np.float64),
                T_cur_w=((n_pairs, 12), np.float64), point_w=((n_pairs, n_pts, 3), np.float64), point_ok=((n_pairs, n_pts), np.uint8),
                result=((n_pairs,), np.int32))


def relative_difference(got, want):
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want)) / max(1.0, float(np.max(np.abs(want))))) if want.size else 0.0


def compare(b, got, bound):
    """got: name -> array over the batch.  Discrete outputs equal on every pair and point; continuous ones within `bound`
    (relative to the larger of 1 and the output's largest magnitude in the pair) where the checker's singular-value
    gaps are at least MIN_GAP.  Returns the largest relative difference per continuous output."""
    assert bound <= 1e-6
    worst = {k: 0.0 for k in CONTINUOUS}
    for i, e in enumerate(b.expect):
        for k in DISCRETE:
            assert np.array_equal(np.asarray(got[k][i]), np.asarray(e[k])), (b.name, i, k, got[k][i], e[k])
        assert np.isfinite(np.concatenate([np.ravel(got[k][i]) for k in CONTINUOUS])).all() or not np.isfinite(e["scale"]), (b.name, i)
        if e["status"] == chk.NO_MODEL:
            assert got["best_hypothesis"][i] == -1
        lost = b.pairs[i].status == 0
        for k in ("xyz_in_cur", "point_w"):
            assert (got[k][i][lost] == 0).all() and (got[k][i][got["inlier"][i] == 0] == 0).all(), (b.name, i, k)
        if e["result"] != chk.SUCCESS:   # the defined zeros past the step that failed (the checker holds them too)
            for k in ("depth_median", "scale", "T_cur_w", "point_w", "point_ok"):
                assert not np.any(got[k][i]), (b.name, i, k)
        if e["status"] != chk.OK:
            for k in ("T_cur_from_ref", "xyz_in_cur", "inlier", "n_inliers", "ambiguous"):
                assert not np.any(got[k][i]), (b.name, i, k)
        if e["status"] == chk.NO_MODEL:
            assert not np.any(got["H"][i]) and not np.any(got["inlier_H"][i])
        if e["gaps"] is None or min(e["gaps"]) < MIN_GAP:
            continue
        for k in CONTINUOUS:
            d = relative_difference(got[k][i], e[k])
            worst[k] = max(worst[k], d)
            assert d <= bound, (b.name, i, k, d)
    return worst
