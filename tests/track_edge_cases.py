"""TEST INFRASTRUCTURE.  Scenes on which svo_hip_find_match_direct, svo_hip_find_epipolar_match_direct and
svo_hip_update_seeds* leave the paths every other chain test stays on (synth.make_track_scene: feature level 0, search
level 0, no feature near a border, A_cur_ref close to the identity, lines of at most 53 positions), a classifier in plain
numpy that says which path of warp_group.h / depth_filter.hip / epi_scan.h a trial or seed takes.  A scene becomes a
tests/tracking_cases.py Case, whose rules (verify_*) tests/test_track_edges_emulated.py and tests/test_track_edges_gpu.py apply.
Everything a case expects -- results, classes, coverage -- comes from the checker (oracle.pytrack) and the classifier;
neither calls the library under test.

A scene is built from synth.make_texture, render, select_features and features_3d on a trajectory of its own: four
keyframes looking down from about 2 m and a current frame placed against them.  Knobs (CASES): camera, feature margin,
per-point feature level, keyframe heights, pose of the current frame (height factor, lateral shift, roll), the depth
intervals of the queries and seeds; SVO_TEST_FUZZ moves the scene's noise and the seeds (helpers.FUZZ, fuzz_rng).  About
400 points and 5 pyramid levels each:

  L   levels.  Feature levels cycle 0 to 3, keyframes at 0.7, 1.0, 1.2 and 1.0 of the height, the current frame at 0.45
      (L05: with 0.6 the distorted cameras' compression keeps det A_cur_ref under 3 for all but the highest keyframe;
      no roll, features from the middle of the keyframes so that they stay in view) and at 1.0 (L10).  Every point is
      seen from its own keyframe alone, or the matcher's closest-view rule would pick the keyframe at the current
      frame's height every time.  Coverage over both poses together.
  Z   zoom out and roll: the current frame at twice the height, rolled 45 degrees, levels {0, 2}: the source box of a
      level-0 feature has about 28 rows, the gather path.
  B   borders: 80 of a keyframe's 100 features from strips 4 to 20 px inside its borders (select_features on the strip),
      the levels of L, the current frame at 1.6 of the height, rolled 45 degrees and shifted 1.2 m so that part of the
      points project near or beyond its border; 24 features whose pixel lies 14 to 40 px OUTSIDE the keyframe (a legal
      call: the whole source box is outside the level, the all-zero patch).
  E   long lines: shift 0.5 m at 0.62 of the height, depth intervals of the queries from 0.0005 to 0.6 of the depth
      (log-uniform, every third one in 0.5 ... 0.6), seeds with depth_min from 100 to 0.15 of the depth; also run with
      max_epi_search_steps = 200.

COVERAGE (assert_coverage; at SVO_TEST_FUZZ=0, where the knobs were chosen): per class a group of cases exists for, at
least 20 members on which the checker succeeds (matcher: ok; query: ok; seed: UPDATED or CONVERGED), at least 10 members
of a class that is itself a rejection.  "lines" counts the queries of find_epipolar_match_direct and the seeds of
update_seeds together: both run seed_prepare_kernel and epi_scan_kernel.

DROPPED CLASSES, with their counts (members/successes):
  * the clamped box in the MATCHER's warp_kernel: 10/1 (pinhole), 13/3 (radtan), 17/5 (atan) in case B.  The
    reference-side rule asks for 6 px at the feature's level and the box reaches 5 px * |A_ref_cur| * 2^search level:
    the trials whose box would be clamped are the ones the rule rejects (253 to 275 of 424).  The same function
    (warp_patch_group8) takes the clamped path in epi_scan_kernel on 321 to 369 lines of case B, 27 to 78 of them
    successful, and that is the class asserted.
  * the per-lane fetch of the scan (epi_scan.h:326) through the C ABI: 21/15 lines on the ATAN camera in case E, none
    on the other two.  tests/test_scan_emulated.py reaches it on 67 and 71 seeds of 480 (emulation only).
  * a box per half group on the radial-tangential camera: 9/8 lines; asserted on the ATAN camera (70/61).

MEASURED CLASS COUNTS at SVO_TEST_FUZZ=0, members/successes; levels are (reference level, search level), warp the path
of warp_group.h:71-83 and 107, bucket depth_filter.hip:273-275, pass the kinds of epi_scan.h:256-257 and 276 that occur
on a line ("none": a pass in which no position is new and inside the frame), mode "cap": a line of more than 1000 steps:

L pinhole (800 points):
  matcher: levels (0, 0) 120/107, (0, 1) 60/37, (1, 0) 25/24, (1, 1) 95/86, (1, 2) 60/32, (2, 1) 25/20, (2, 2) 95/80,
    (2, 3) 60/30, (3, 2) 23/17, (3, 3) 108/79, (3, 4) 120/51; warp lds_inside 791/563; rejected by the border rule 9
    (9 above level 0)
  lines: levels (0, 0) 174/165, (0, 1) 77/46, (0, 2) 1/0, (1, 0) 36/34, (1, 1) 133/128, (1, 2) 75/50, (1, 3) 3/2, (2,
    1) 40/40, (2, 2) 144/129, (2, 3) 76/48, (2, 4) 1/0, (3, 2) 36/36, (3, 3) 152/135, (3, 4) 158/71; warp lds_clamped
    3/1, lds_inside 1103/883; mode cap 12/0, scan 708/566, short 386/318; bucket 0 170/139, 1 149/132, 2 154/119, 3
    116/98, 4 66/46, 5 19/13, 6 23/11, 7 11/8; pass none 237/108, one 621/566
L radtan (800 points):
  matcher: levels (0, 0) 140/122, (0, 1) 34/25, (0, 2) 5/0, (0, 3) 1/0, (1, 0) 15/14, (1, 1) 124/105, (1, 2) 35/25,
    (1, 3) 5/0, (1, 4) 1/0, (2, 1) 16/11, (2, 2) 119/97, (2, 3) 40/24, (2, 4) 5/0, (3, 2) 14/8, (3, 3) 132/97, (3, 4)
    95/33; warp gather 3/0, lds_inside 778/561; rejected by the border rule 19 (19 above level 0)
  lines: levels (0, 0) 217/192, (0, 1) 40/21, (0, 2) 2/0, (0, 3) 1/0, (0, 4) 1/0, (1, 0) 23/23, (1, 1) 183/164, (1, 2)
    43/35, (1, 3) 8/1, (1, 4) 1/0, (2, 1) 27/27, (2, 2) 202/183, (2, 3) 51/33, (2, 4) 5/1, (3, 2) 25/24, (3, 3)
    224/164, (3, 4) 115/33; warp gather 4/0, lds_clamped 7/4, lds_inside 1157/897; mode cap 70/0, scan 686/558, short
    412/343; bucket 0 171/143, 1 148/122, 2 169/138, 3 109/88, 4 52/46, 5 19/12, 6 13/6, 7 5/3; pass half 3/3, none
    180/71, one 608/558
L atan (800 points):
  matcher: levels (0, 0) 157/140, (0, 1) 23/21, (1, 0) 11/11, (1, 1) 146/117, (1, 2) 23/20, (2, 1) 11/7, (2, 2)
    143/109, (2, 3) 26/19, (3, 2) 8/5, (3, 3) 168/99, (3, 4) 53/36; warp lds_inside 769/584; rejected by the border
    rule 31 (31 above level 0)
  lines: levels (0, 0) 238/201, (0, 1) 30/22, (1, 0) 16/15, (1, 1) 211/195, (1, 2) 27/26, (1, 3) 1/1, (2, 1) 18/18,
    (2, 2) 224/198, (2, 3) 35/27, (3, 2) 19/16, (3, 3) 267/171, (3, 4) 69/45; warp lds_clamped 15/0, lds_inside
    1140/935; mode cap 2/0, scan 731/591, short 422/344; bucket 0 184/141, 1 163/129, 2 150/134, 3 123/97, 4 64/57, 5
    26/18, 6 20/14, 7 1/1; pass half 22/17, lane 18/11, none 239/123, one 657/585
Z pinhole (400 points):
  matcher: levels (0, 0) 200/184, (2, 1) 200/184; warp gather 200/184, lds_inside 200/184; rejected by the border rule
    0 (0 above level 0)
  lines: levels (0, 0) 324/313, (2, 0) 6/3, (2, 1) 295/293; warp gather 324/313, lds_inside 301/296; mode scan
    420/418, short 205/191; bucket 0 48/48, 1 80/80, 2 143/141, 3 117/117, 4 32/32; pass none 5/5, one 420/418
Z radtan (400 points):
  matcher: levels (0, 0) 200/180, (2, 1) 198/160; warp gather 190/171, lds_inside 208/169; rejected by the border rule
    2 (2 above level 0)
  lines: levels (0, 0) 336/318, (2, 1) 320/298; warp gather 322/304, lds_inside 334/312; mode scan 447/435, short
    209/181; bucket 0 8/8, 1 67/65, 2 111/107, 3 163/157, 4 98/98; pass none 20/12, one 444/435
Z atan (400 points):
  matcher: levels (0, 0) 200/184, (2, 1) 196/156; warp gather 182/174, lds_inside 214/166; rejected by the border rule
    4 (4 above level 0)
  lines: levels (0, 0) 329/304, (2, 1) 312/278, (2, 2) 1/1; warp gather 307/286, lds_inside 335/297; mode scan
    440/413, short 202/170; bucket 0 8/8, 1 71/65, 2 109/104, 3 157/144, 4 95/92; pass none 29/13, one 435/413
B pinhole (424 points):
  matcher: levels (0, 0) 90/56, (1, 0) 54/45, (2, 1) 15/14, (3, 2) 12/8; warp gather 84/56, lds_clamped 10/1,
    lds_inside 77/66; rejected by the border rule 253 (219 above level 0)
  lines: levels (0, 0) 173/77, (1, 0) 138/75, (2, 1) 140/33, (3, 2) 140/16; warp gather 126/75, lds_clamped 321/27,
    lds_inside 110/99, zeros 34/0; mode scan 408/147, short 183/54; bucket 0 45/7, 1 64/13, 2 77/24, 3 108/41, 4
    73/35, 5 41/27; pass none 59/0, one 355/147
B radtan (424 points):
  matcher: levels (0, 0) 84/48, (1, 0) 47/35, (1, 1) 4/2, (2, 1) 12/9, (2, 2) 2/2, (3, 2) 6/5; warp gather 49/29,
    lds_clamped 13/3, lds_inside 93/69; rejected by the border rule 269 (229 above level 0)
  lines: levels (0, 0) 189/97, (1, 0) 134/78, (1, 1) 6/2, (2, 1) 142/43, (2, 2) 9/4, (3, 2) 138/25, (3, 3) 8/3; warp
    gather 94/61, lds_clamped 369/78, lds_inside 128/113, zeros 35/0; mode scan 434/184, short 192/68; bucket 0 57/21,
    1 71/24, 2 82/23, 3 107/46, 4 59/26, 5 55/42, 6 3/2; pass none 77/10, one 387/184
B atan (424 points):
  matcher: levels (0, 0) 79/46, (1, 0) 24/18, (1, 1) 29/20, (2, 1) 8/8, (2, 2) 3/1, (3, 2) 3/2, (3, 3) 3/1; warp
    gather 18/10, lds_clamped 17/5, lds_inside 114/81; rejected by the border rule 275 (230 above level 0)
  lines: levels (0, 0) 180/89, (1, 0) 59/28, (1, 1) 78/43, (2, 1) 61/19, (2, 2) 83/16, (3, 2) 59/5, (3, 3) 85/4; warp
    gather 42/27, lds_clamped 366/46, lds_inside 162/131, zeros 35/0; mode scan 418/144, short 187/60; bucket 0 50/7,
    1 67/17, 2 104/25, 3 93/39, 4 61/26, 5 40/27, 6 3/3; pass none 136/14, one 334/144
E pinhole (400 points):
  matcher: levels (0, 0) 300/164, (1, 1) 100/52; warp lds_inside 400/216; rejected by the border rule 0 (0 above level
    0)
  lines: levels (0, 0) 322/180, (0, 1) 49/18, (1, 1) 112/72, (1, 2) 13/7; warp lds_inside 496/277; mode cap 107/0,
    scan 348/253, short 41/24; bucket 0 33/20, 1 35/20, 2 36/26, 3 44/32, 4 47/30, 5 45/32, 6 46/38, 7 62/55; pass
    none 187/107, one 293/253
E radtan (400 points):
  matcher: levels (0, 0) 280/216, (0, 1) 20/4, (1, 1) 98/73, (1, 2) 2/1; warp lds_inside 400/294; rejected by the
    border rule 0 (0 above level 0)
  lines: levels (0, 0) 388/254, (0, 1) 34/12, (0, 3) 1/0, (1, 1) 132/92, (1, 2) 8/6, (1, 3) 1/0; warp gather 1/0,
    lds_inside 563/364; mode cap 122/0, scan 363/304, short 79/60; bucket 0 53/37, 1 36/32, 2 47/38, 3 42/35, 4 53/45,
    5 62/54, 6 47/43, 7 23/20; pass half 9/8, none 140/95, one 331/304
E atan (400 points):
  matcher: levels (0, 0) 296/217, (0, 1) 4/4, (1, 1) 100/65; warp lds_inside 400/286; rejected by the border rule 0 (0
    above level 0)
  lines: levels (0, 0) 402/317, (0, 1) 19/11, (1, 1) 125/100, (1, 2) 7/6; warp lds_inside 553/434; mode cap 12/0, scan
    447/359, short 94/75; bucket 0 48/44, 1 33/23, 2 47/37, 3 49/39, 4 55/44, 5 89/73, 6 92/71, 7 34/28; pass half
    70/61, lane 21/15, none 224/147, one 392/343
"""
import ctypes as C
import functools

import numpy as np
import torch

from helpers import FUZZ, camera_models
from oracle import pyoracle, pytrack
from rpg_svo_amd import se3, synth
from tracking_cases import DEFAULT_SEED_MIN, DEFAULT_SPREADS, N_LEVELS, OK_SEED, Case

N_KF, N_FEAT = 4, 100
HEIGHT = 2.0
MIN_OK, MIN_REJECTED = 20, 10     # coverage: successes per class / members of a class that is itself a rejection
SCAN_G, SCAN_PP, SCAN_BUCKETS, BOX_ROWS = 8, 16, 8, 20   # epi_scan.h, warp_group.h

# name -> knobs of a scene.  poses: (height factor, lateral shift [m], direction of the shift [deg], roll [deg]) of the
# current frame against the keyframes; spreads: relative half width of a query's depth interval; seed_min: depth_min of a
# seed as a fraction of its depth (z_range = 1 / depth_min, sigma = z_range / 6)
def _log_cycle(lo, hi, skew=1.0, top=None, n=400):
    """n values between lo and hi, log-uniform (golden-ratio sequence): line lengths then fall evenly over the power-of-two
    buckets of the scan; with `top` every third value lies in that interval instead (the longest lines)"""
    u = lambda i: (i * 0.6180339887498949) % 1.0
    return tuple(float(top[0] + (top[1] - top[0]) * u(i) ** skew) if top and i % 3 == 0 else float(lo * (hi / lo) ** (u(i) ** skew)) for i in range(n))


CASES = {
    "L05": dict(levels=(0, 1, 2, 3, 3), kf_heights=(0.7, 1.0, 1.2, 1.0), pose=(0.45, 0.0, 30.0, 0.0), margin=150, cell=20, single_every=1),
    "L10": dict(levels=(0, 1, 2, 3), kf_heights=(0.7, 1.0, 1.2, 1.0), pose=(1.0, 0.1, 30.0, 0.0), margin=40, single_every=1),
    "Z": dict(levels=(0, 2), kf_heights=(1.0, 1.0, 1.05, 0.95), pose=(2.0, 0.15, 200.0, 45.0), margin=40),
    "B": dict(levels=(0, 1, 2, 3), kf_heights=(0.8, 0.9, 1.0, 0.8), pose=(1.6, 1.2, 10.0, 45.0), margin=4, strips=True, ghosts=24),
    "E": dict(levels=(0, 0, 0, 1), kf_heights=(1.0, 1.0, 1.05, 0.95), pose=(0.62, 0.5, 0.0, 0.0), margin=110, cell=24,
              spreads=_log_cycle(0.0005, 0.6, 0.5, (0.5, 0.6)), seed_min=_log_cycle(100.0, 0.2, 0.5, (0.15, 0.2)), cap=200),
}


class Scene:
    """cam, T_f_w [K+1,12] (row K: the current frame), images [K+1,h,w] u8, cur, T_cur_prior, pt_pos [P,3], obs (per point:
    [(frame, px, f, level, type, grad)]), px_init [P,2], feats (per point: the feature of its seed / query), d_true [P]"""


def _rot(rv):
    return se3.split(se3.exp(np.concatenate([np.zeros(3), rv])))[0]


def _pose(centre, rv):
    R = _rot(rv) @ np.diag([1.0, -1.0, -1.0])   # the camera looks down; rv turns it in its own frame (z: the optical axis)
    return se3.join(R, -R @ np.asarray(centre, np.float64))


def _strip_features(images, n, margin, band=24, cell=8):
    """n // 4 features per border strip of `band` pixels (select_features on the strip alone): [K, 4 (n // 4), 2]"""
    k, h, w = images.shape
    q = n // 4
    out = []
    for crop, off in ((images[:, :, :band], (0, 0)), (images[:, :, w - band:], (w - band, 0)), (images[:, :band, :], (0, 0)),
                      (images[:, h - band:, :], (0, h - band))):
        p = synth.select_features(crop.contiguous(), q, margin=margin, cell=cell).cpu().numpy()
        out.append(p + np.array(off, np.float64))
    return np.concatenate(out, axis=1)


def build_scene(cam, levels, kf_heights, pose, margin, cell=32, strips=False, ghosts=0, single_every=0, depth_noise=0.01, prior_noise=2e-3, edgelet_frac=0.25, **_):
    rng = np.random.default_rng(777 + FUZZ)
    K = N_KF
    xy = np.array([(-0.15, -0.1), (0.1, -0.12), (0.12, 0.1), (-0.1, 0.12)]) + rng.normal(0, 0.02, (K, 2))
    T = np.zeros((K + 1, 12))
    for k in range(K):
        T[k] = _pose([xy[k, 0], xy[k, 1], HEIGHT * kf_heights[k]], rng.normal(0, 0.02, 3))
    hf, shift, sdir, roll = pose
    c_cur = [shift * np.cos(np.radians(sdir)), shift * np.sin(np.radians(sdir)), HEIGHT * hf]
    T[K] = _pose(c_cur, np.array([rng.normal(0, 0.01), rng.normal(0, 0.01), np.radians(roll)]))
    images = synth.render(synth.make_texture(seed=12345), T, cam)
    px_kf = synth.select_features(images[:K], N_FEAT, margin=max(margin, 4), cell=cell).cpu().numpy()
    if strips:
        n_strip = 80
        px_kf[:, :n_strip] = _strip_features(images[:K], n_strip, margin)
    px_kf = px_kf + rng.uniform(-0.5, 0.5, size=px_kf.shape)
    imgs = images.cpu().numpy()
    imf = imgs.astype(np.float32)
    h, w = imgs.shape[1:]
    obs_margin = min(12, margin)
    s = Scene()
    pts, obs_all, feats = [], [], []

    def grad_at(k, p):
        ju, jv = int(np.clip(round(p[0]), 1, w - 2)), int(np.clip(round(p[1]), 1, h - 2))
        gx, gy = imf[k, jv, ju + 1] - imf[k, jv, ju - 1], imf[k, jv + 1, ju] - imf[k, jv - 1, ju]
        return gx, gy, float(np.hypot(gx, gy))

    for k in range(K):
        px_k = px_kf[k]
        if ghosts and k == 0:   # features whose pixel lies outside the keyframe: the whole source box of the warp is outside
            g = np.stack([-rng.uniform(14, 40, ghosts), rng.uniform(60, h - 60, ghosts)], -1)
            g[ghosts // 2:] = np.stack([rng.uniform(60, w - 60, ghosts - ghosts // 2), h + rng.uniform(14, 40, ghosts - ghosts // 2)], -1)
            px_k = np.concatenate([px_k, g])
        f_k, X_k = synth.features_3d(T[k:k + 1], cam, torch.as_tensor(px_k[None]))
        f_k, X_k = f_k[0].numpy(), X_k[0].numpy()
        c_k = -T[k, :9].reshape(3, 3).T @ T[k, 9:]
        for i in range(len(px_k)):
            ghost = i >= N_FEAT
            level = 0 if ghost else levels[(k * N_FEAT + i) % len(levels)]
            X = X_k[i]
            Xn = c_k + (X - c_k) * (1.0 + depth_noise * rng.normal())
            gx, gy, gn = grad_at(k, px_k[i])
            is_edge = bool(rng.uniform() < edgelet_frac and gn > 1e-3 and not ghost)
            grad = (gx / gn, gy / gn) if is_edge else (1.0, 0.0)
            o = [(k, px_k[i].copy(), f_k[i].copy(), level, 1 if is_edge else 0, grad)]
            for k2 in range(K):
                if k2 == k or ghost or (strips and i < 80) or (single_every and i % single_every == 0):   # (seen from its own keyframe alone: the matcher must take it)
                    continue
                p2, z2 = synth._proj(T[k2], cam, X[None])
                if z2[0] > 0 and obs_margin <= p2[0, 0] < w - obs_margin and obs_margin <= p2[0, 1] < h - obs_margin:
                    g2 = (1.0, 0.0)
                    if is_edge:
                        hx, hy, hn = grad_at(k2, p2[0])
                        g2 = (hx / hn, hy / hn) if hn > 1e-3 else grad
                    o.append((k2, p2[0].copy(), synth._bearing(cam, p2)[0], level, 1 if is_edge else 0, g2))
            if synth._proj(T[K], cam, X[None])[1][0] <= 0:
                continue
            order = rng.permutation(len(o))
            pts.append(Xn)
            obs_all.append([o[j] for j in order])
            feats.append(o[0])
    s.cam, s.T_f_w, s.images, s.cur = cam, T, imgs, K
    s.pt_pos = np.array(pts)
    s.obs, s.feats = obs_all, feats
    s.T_cur_prior = se3.mul(se3.exp(rng.normal(size=6) * prior_noise), T[K])
    s.px_init, _ = synth._proj(s.T_cur_prior, cam, s.pt_pos)
    c_ref = np.array([-T[o[0], :9].reshape(3, 3).T @ T[o[0], 9:] for o in feats])
    s.d_true = np.linalg.norm(s.pt_pos - c_ref, axis=1)
    return s


# ---- the classifier (plain numpy: restates the conditions, never calls the library under test) ----------------------------
def oracle_world2cam(cam):
    """uv [n,2] -> px [n,2] through the oracle's world2cam (orc_reproject_point of (u, v, 1) under the identity pose: the
    function tests/test_device_math_host.py pins device_math.h against)"""
    lib, pc = pyoracle.lib(), pyoracle.make_cam(cam)
    D = C.POINTER(C.c_double)
    T = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)
    xyz, out = np.ones(3), np.zeros(2)
    pT, pxyz, pout, ppc = T.ctypes.data_as(D), xyz.ctypes.data_as(D), out.ctypes.data_as(D), C.byref(pc)
    fn = lib.orc_reproject_point

    def f(uv):
        res = np.empty((len(uv), 2))
        for i in range(len(uv)):
            xyz[0], xyz[1] = uv[i, 0], uv[i, 1]
            fn(ppc, pT, pxyz, 30, 26, pout)
            res[i] = out
        return res
    f._keep = (pc, T, xyz, out)
    return f


def warp_path(A_cur_ref, px_ref, level, sl, cols, rows):
    """warp_group.h:56-83, 107: "zeros" / "lds_inside" / "lds_clamped" / "gather" of one trial, from A_cur_ref (f64 2 x 2), the
    feature's pixel and level, the search level and the size of the reference level"""
    f = np.float32
    A = np.asarray(A_cur_ref, np.float64).reshape(2, 2)
    det = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
    with np.errstate(all="ignore"):
        inv = np.array([A[1, 1], -A[0, 1], -A[1, 0], A[0, 0]]) / det
        Ax, Ay, Az, Aw = (f(v) for v in inv)
        pyrx, pyry = f(px_ref[0]) * f(1.0 / (1 << level)), f(px_ref[1]) * f(1.0 / (1 << level))
        sc = f(1 << sl)
        if np.isnan(Ax):
            return "zeros"
        q0, q1 = [], []
        for k in range(4):
            pp0, pp1 = f(4 if k & 1 else -5) * sc, f(4 if k & 2 else -5) * sc
            q0.append(f(f(Ax * pp0) + f(Ay * pp1)) + pyrx)
            q1.append(f(f(Az * pp0) + f(Aw * pp1)) + pyry)
    bx0, bx1, by0, by1 = min(q0), max(q0), min(q1), max(q1)
    if not (bx0 > -1.0e6 and bx1 < 1.0e6 and by0 > -1.0e6 and by1 < 1.0e6 and bx0 <= bx1 and by0 <= by1):
        return "gather"
    xhi, yhi = int(np.floor(bx1)) + 1, int(np.floor(by1)) + 1
    xlo, ylo = max(int(np.floor(bx0)), 0), max(int(np.floor(by0)), 0)
    xhi, yhi = min(xhi, cols - 1), min(yhi, rows - 1)
    cx0 = xlo & ~15
    nch = ((xhi - cx0) >> 4) + 1 if xhi >= cx0 else 0
    nrow = yhi - ylo + 1
    if xhi < xlo or yhi < ylo:
        return "zeros"
    if nch <= 3 and nrow <= BOX_ROWS and nrow * nch <= 6 * 8:
        all_in = bx0 >= 0 and by0 >= 0 and bx1 < f(cols - 1) and by1 < f(rows - 1)
        return "lds_inside" if all_in else "lds_clamped"
    return "gather"


def scan_bucket(n_steps, scanned=True):
    """depth_filter.hip:273-275"""
    n_pos = n_steps + 1 if scanned else 1
    passes = (n_pos + SCAN_PP - 1) // SCAN_PP
    return 0 if n_pos <= SCAN_G else min(SCAN_BUCKETS - 1, 1 + (0 if passes <= 1 else int(passes - 1).bit_length()))


def _box_fits(xs, ys):
    """epi_scan.h:273-276 for the windows [x-4, x+3] x [y-4, y+3] of the wanted positions xs, ys (not empty)"""
    x_lo, x_hi, y_lo, y_hi = xs.min() - 4, xs.max() + 3, ys.min() - 4, ys.max() + 3
    n_rows, n_cols = y_hi - y_lo + 1, ((x_hi - (x_lo & ~15)) >> 4) + 1
    return n_rows <= BOX_ROWS and n_cols <= 3 and n_rows * n_cols <= 48


def scan_pass_kinds(px, sl, width, height, offsets=None):
    """Per pass of a line whose positions project to px [n,2] (level 0): "none" (nothing wanted), "one" (one box for the
    group, epi_scan.h:256-257), "half" (a box per half group), "lane" (a half group whose box does not fit either: the
    per-lane fetch, :276 and :326).  offsets: a set that receives the offset of every box inside its first tile column."""
    with np.errstate(invalid="ignore"):
        p = np.trunc(px / (1 << sl) + 0.5)
    p = np.where(np.isfinite(p) & (np.abs(p) < 2 ** 31), p, -2.0 ** 31).astype(np.int64)
    prev = np.vstack([[0, 0], p[:-1]])
    wl, hl = width // (1 << sl), height // (1 << sl)
    want = (p != prev).any(axis=1) & (p[:, 0] >= 8) & (p[:, 0] < wl - 8) & (p[:, 1] >= 8) & (p[:, 1] < hl - 8)
    n = len(p)
    per = SCAN_G if n <= SCAN_G else SCAN_PP
    kinds = []
    for b in range(0, n, per):
        halves = [np.flatnonzero(want[b + h * per // 2:min(b + (h + 1) * per // 2, n)]) + b + h * per // 2 for h in (0, 1)]
        idx = np.concatenate(halves)
        if len(idx) == 0:
            kinds.append("none")
        elif _whole(p[idx, 0], p[idx, 1]):
            kinds.append("one")
            boxes = [idx]
        elif all(len(hx) == 0 or _box_fits(p[hx, 0], p[hx, 1]) for hx in halves):
            kinds.append("half")
            boxes = [hx for hx in halves if len(hx)]
        else:
            kinds.append("lane")
            boxes = [hx for hx in halves if len(hx) and _box_fits(p[hx, 0], p[hx, 1])]
        if offsets is not None and kinds[-1] != "none":
            offsets.update(int((p[bx, 0].min() - 4) & 15) for bx in boxes)
    return kinds


def _whole(xs, ys):
    gx_lo, gx_hi, gy_lo, gy_hi = xs.min() - 4, xs.max() + 3, ys.min() - 4, ys.max() + 3
    return gy_hi - gy_lo < BOX_ROWS and gx_hi - (gx_lo & ~15) < 48 and (gy_hi - gy_lo + 1) * (((gx_hi - (gx_lo & ~15)) >> 4) + 1) <= 48


def line_uv(T_ref, T_cur, f, d_min, d_max, n_steps):
    """the positions of matcher.cpp:264-268 on the unit plane: B - step, then n_steps sequential additions of step"""
    T_cur_ref = se3.mul(T_cur, se3.inv(T_ref))
    R, t = se3.split(T_cur_ref)
    qa, qb = R @ (f * d_min) + t, R @ (f * d_max) + t
    A, B = qa[:2] / qa[2], qb[:2] / qb[2]
    step = (A - B) / n_steps
    return np.cumsum(np.vstack([B - step, np.tile(step, (n_steps, 1))]), axis=0)


# ---- a case: a scene of build_scene as a tracking_cases.Case, and its classes (orc checker + classifier) ---------------------
def _level_size(c, level):
    return c.scene.images.shape[2] >> level, c.scene.images.shape[1] >> level


def matcher_classes(c):
    """per trial: dict(ok, levels=(ref level, search level) or None, warp, border_rejected)"""
    def run():
        s, out = c.scene, []
        for i, (ok, _, r) in enumerate(c.matcher_ref()):
            o = s.obs[i][r["ref_obs"]]
            rl = o[3]
            wl, hl = s.cam.width // (1 << rl), s.cam.height // (1 << rl)
            x, y = int(o[1][0]) // (1 << rl), int(o[1][1]) // (1 << rl)   # (int(): towards zero, as the cast)
            if o[1][0] < 0 or o[1][1] < 0:
                x, y = -1, -1
            inside = 6 <= x < wl - 6 and 6 <= y < hl - 6
            reached = bool(r["A_cur_ref"].any())
            assert reached <= inside
            d = dict(ok=ok, levels=None, warp=None, border_rejected=not inside, ref_level=rl)
            if reached:
                d["levels"] = (rl, r["search_level"])
                d["warp"] = warp_path(r["A_cur_ref"], o[1], rl, r["search_level"], *_level_size(c, rl))
            out.append(d)
        return out
    return c._memo("matcher_classes", run)


def line_classes(c, kind):
    """kind "epi" (the queries) or "seeds".  per entry: dict(ok, levels, warp, mode: "none" / "short" / "scan" / "cap",
    n_steps, bucket, passes: set of pass kinds) -- the line itself from the checker's findEpipolarMatchDirect on the
    entry's depth interval (A_cur_ref, search level, epi_length)"""
    def run():
        s = c.scene
        orc, _, _, ft = c.checker("orc")
        w2c = oracle_world2cam(s.cam)
        opt = pytrack.matcher_options(n_pyr_levels=N_LEVELS)
        out = []
        if kind == "epi":
            res = c.epi_ref()
            oks = [ok for ok, _ in res]
            lines = [(c.epi.d_est[k], c.epi.d_min[k], c.epi.d_max[k], res[k][1]) for k in range(c.P)]
        else:
            so, io = c.seeds_ref()
            oks = [x.status in OK_SEED for x in io]
            lines = []
            sc = c.seed_cols
            for k in range(c.P):
                if io[k].status in (pytrack.SEED_ERASED_OLD, pytrack.SEED_BEHIND, pytrack.SEED_NOT_IN_FRAME):
                    lines.append(None)
                    continue
                mu, sq = sc["mu"][k], np.sqrt(sc["sigma2"][k])
                zlo = np.float32(mu - sq)
                d = (1.0 / float(mu), 1.0 / float(np.float32(mu + sq)), 1.0 / float(zlo if zlo >= np.float32(1e-8) else np.float32(1e-8)))
                _, r = orc.find_epipolar_match_direct(ft, s.cam, c.feats[k][0], s.cur, pytrack.make_feature(*c.feats[k]), *d, opt)
                lines.append((*d, r))
        for k in range(c.P):
            d = dict(ok=bool(oks[k]), levels=None, warp=None, mode="none", n_steps=0, bucket=None, passes=set())
            if lines[k] is not None and not lines[k][3]["reject"]:
                de, dmin, dmax, r = lines[k]
                o = c.feats[k]
                sl = r["search_level"]
                d["levels"] = (o[3], sl)
                d["warp"] = warp_path(r["A_cur_ref"], o[1], o[3], sl, *_level_size(c, o[3]))
                el = r["epi_length"]
                if el < 2.0:
                    d["mode"], d["bucket"] = "short", 0
                elif not np.isfinite(el) or int(el / 0.7) > 1000:
                    d["mode"], d["n_steps"] = "cap", (int(el / 0.7) if np.isfinite(el) else -1)
                else:
                    n = int(el / 0.7)
                    d["mode"], d["n_steps"], d["bucket"] = "scan", n, scan_bucket(n)
                    uv = line_uv(s.T_f_w[o[0]], s.T_f_w[s.cur], o[2], dmin, dmax, n)
                    d["passes"] = set(scan_pass_kinds(w2c(uv), sl, s.cam.width, s.cam.height))
            out.append(d)
        return out
    return c._memo(("line_classes", kind), run)


def counts(c):
    """the class counts of the docstring: name -> (members, of which the checker succeeds)"""
    def run():
        cnt = {}

        def add(key, ok):
            m, n = cnt.get(key, (0, 0))
            cnt[key] = (m + 1, n + int(bool(ok)))
        for d in matcher_classes(c):
            if d["border_rejected"]:
                add("match border-rejected", False)
                if d["ref_level"] > 0:
                    add("match border-rejected above level 0", False)
            if d["levels"]:
                add(f"match levels {d['levels']}", d["ok"])
                add(f"match sl {d['levels'][1]}", d["ok"])
                add("match sl " + ("above" if d["levels"][1] > d["levels"][0] else "equal" if d["levels"][1] == d["levels"][0] else "below") + " ref", d["ok"])
                add(f"match warp {d['warp']}", d["ok"])
        for kind in ("epi", "seeds"):
            for d in line_classes(c, kind):
                if not d["levels"]:
                    continue
                add(f"{kind} levels {d['levels']}", d["ok"])
                add(f"{kind} sl {d['levels'][1]}", d["ok"])
                add(f"{kind} sl " + ("above" if d["levels"][1] > d["levels"][0] else "equal" if d["levels"][1] == d["levels"][0] else "below") + " ref", d["ok"])
                add(f"{kind} warp {d['warp']}", d["ok"])
                add(f"{kind} mode {d['mode']}", d["ok"])
                if d["mode"] == "scan":
                    add(f"{kind} bucket {d['bucket']}", d["ok"])
                    for p in d["passes"]:
                        add(f"{kind} pass {p}", d["ok"])
        return cnt
    return c._memo("counts", run)


@functools.lru_cache(maxsize=None)
def case(name, cam_kind):
    k = CASES[name]
    s = build_scene(camera_models()[cam_kind], **k)
    c = Case(name, s, s.feats, s.d_true, spreads=k.get("spreads", DEFAULT_SPREADS), seed_min=k.get("seed_min", DEFAULT_SEED_MIN), cap=k.get("cap"),
             cam_kind=cam_kind, knobs=k)
    c.describe = lambda kind, i: (matcher_classes(c) if kind == "matcher" else line_classes(c, kind))[i]
    return c


def format_counts(cnt):
    return "; ".join(f"{k}: {m} ({n} ok)" for k, (m, n) in sorted(cnt.items()))


# ---- coverage: on the checker and the classifier alone ---------------------------------------------------------------------
# group -> (the cases whose counts are added up, [(class, minimum of successes)], [(rejection class, minimum of members)]).
# "lines" are the queries of find_epipolar_match_direct and the seeds of update_seeds together: both run seed_prepare_kernel
# and epi_scan_kernel.
def _lv(prefix):
    return [(f"{prefix} sl {k}", MIN_OK) for k in range(5)] + [(f"{prefix} sl {r} ref", MIN_OK) for r in ("above", "equal", "below")]


COVERAGE = {
    "L": (("L05", "L10"), _lv("match") + _lv("lines"), []),
    "Z": (("Z",), [("match warp gather", MIN_OK), ("lines warp gather", MIN_OK), ("match warp lds_inside", MIN_OK), ("lines warp lds_inside", MIN_OK)], []),
    "B": (("B",), [("lines warp lds_clamped", MIN_OK), ("match warp lds_inside", MIN_OK)],
          [("match border-rejected", MIN_REJECTED), ("match border-rejected above level 0", MIN_REJECTED), ("lines warp zeros", MIN_REJECTED)]),
    "E": (("E",), [(f"lines bucket {k}", MIN_OK) for k in range(SCAN_BUCKETS)] + [("lines mode short", MIN_OK), ("lines pass one", MIN_OK)],
          [("lines mode cap", MIN_REJECTED)]),
}
# the distorted line of the ATAN camera: passes that need a box per half group
COVERAGE_ATAN_E = [("lines pass half", MIN_OK)]


def group_counts(group, cam_kind):
    total = {}
    for name in COVERAGE[group][0]:
        for k, (m, n) in counts(case(name, cam_kind)).items():
            keys = [k]
            if k.startswith(("epi ", "seeds ")):
                keys.append("lines " + k.split(" ", 1)[1])
            for kk in keys:
                a, b = total.get(kk, (0, 0))
                total[kk] = (a + m, b + n)
    return total


def assert_coverage(group, cam_kind):
    """The coverage conditions of a group of cases, at SVO_TEST_FUZZ=0 (the knobs were chosen there).  Prints the counts."""
    cnt = group_counts(group, cam_kind)
    print(f"{group} {cam_kind}: {format_counts(cnt)}")
    if FUZZ:
        return cnt
    _, need_ok, need_members = COVERAGE[group]
    if group == "E" and cam_kind == "atan":
        need_ok = need_ok + COVERAGE_ATAN_E
    for k, n in need_ok:
        assert cnt.get(k, (0, 0))[1] >= n, f"{group} {cam_kind}: class '{k}' has {cnt.get(k, (0, 0))} (members, successes), needs {n} successes"
    for k, n in need_members:
        assert cnt.get(k, (0, 0))[0] >= n, f"{group} {cam_kind}: class '{k}' has {cnt.get(k, (0, 0))[0]} members, needs {n}"
    return cnt
