"""The f64 checker of svo_hip_homography_init (tests/homography_checker.py) against ground truth, on the synthetic
geometry of tests/homography_cases.py.  This is what makes the checker a reference: the device is compared against it
(tests/test_homography_emulated.py, tests/test_homography_gpu.py), and it is compared against the scene."""
import numpy as np
import pytest

import homography_cases as cases
import homography_checker as chk

EXACT_SEEDS = range(300, 312)
NOISY_SEEDS = range(400, 424)


def run(p, **kw):
    return chk.homography_init(p.cam, p.f_ref, p.f_cur, p.status, p.px_ref, p.px_cur, p.T_ref_w, **kw)


def pose_errors(R, t, truth):
    return cases.rotation_angle(R, truth.R), cases.direction_angle(t, truth.t)


def best_finalist(e, truth):
    return min((pose_errors(R, t, truth) for R, t in e["finalists"]), key=lambda rt: max(rt))


@pytest.mark.parametrize("map_scale", [1.0, 2.5])
def test_exact_scenes(map_scale):
    """Relief-free, noise-free planes (200 points, 60 lost ones between them): the chosen pose -- with `ambiguous` set, one of
    the two finalists -- is the true one within 1e-6 rad in rotation and in translation direction, scale * depth_median is
    map_scale, and the map points lie on the true structure, scaled about the reference camera, to 1e-9 relative.
    Measured over the 12 scenes (both map scales): rotation <= 5.0e-16 rad, translation direction <= 3.7e-15 rad, structure
    <= 3.0e-13 relative; none of the 12 pairs is ambiguous (the second-best candidate scores below 0.9 of the best)."""
    worst = np.zeros(3)
    n_ambiguous = 0
    for seed in EXACT_SEEDS:
        p = cases.make_pair(seed, 200, noise=0.0, outliers=0.0, relief=0.0, n_lost=60)
        e = run(p, map_scale=map_scale)
        assert e["status"] == chk.OK and e["result"] == chk.SUCCESS and e["n_inliers"] == 200
        if e["ambiguous"]:
            n_ambiguous += 1
            rot, tra = best_finalist(e, p.truth)
        else:
            rot, tra = pose_errors(e["T_cur_from_ref"][:9].reshape(3, 3), e["T_cur_from_ref"][9:], p.truth)
        assert rot <= 1e-6 and tra <= 1e-6, (seed, rot, tra)
        assert abs(e["scale"] * e["depth_median"] - map_scale) <= 1e-15 * map_scale
        chosen_is_true = max(pose_errors(e["T_cur_from_ref"][:9].reshape(3, 3), e["T_cur_from_ref"][9:], p.truth)) <= 1e-6
        if chosen_is_true:
            # the structure: X_w of the truth, scaled about the reference camera's position by one factor for all points
            R_rw, t_rw = p.T_ref_w[:9].reshape(3, 3), p.T_ref_w[9:]
            pos_ref = -R_rw.T @ t_rw
            on = e["inlier"] != 0
            X_w = (p.truth.X_ref[on] - t_rw) @ R_rw
            a, b = X_w - pos_ref, e["point_w"][on] - pos_ref
            g = (a * b).sum() / (a * a).sum()
            off = np.linalg.norm(b - g * a, axis=1).max() / np.linalg.norm(b, axis=1).max()
            assert off <= 1e-9, (seed, off)
            # and the median depth of the scaled points in the current frame is map_scale
            R_cw, t_cw = e["T_cur_w"][:9].reshape(3, 3), e["T_cur_w"][9:]
            z = np.sort((e["point_w"][on] @ R_cw.T + t_cw)[:, 2])
            assert abs(z[len(z) // 2] - map_scale) <= 1e-12 * map_scale
            worst = np.maximum(worst, [rot, tra, off])
    print(f"exact scenes: rotation {worst[0]:.1e} rad, translation direction {worst[1]:.1e} rad, structure {worst[2]:.1e}; {n_ambiguous} ambiguous")


def test_noisy_scenes():
    """0.3 px noise, 30 % outliers, 3 % relief, 352 tracked points: rotation <= 2e-2 rad, translation direction <= 0.1 rad,
    final inliers >= 0.9 of the true non-outliers (unambiguous pairs; an ambiguous pair is held to the inlier share and to
    "one of the two finalists meets the pose caps").
    Measured over the 24 scenes: rotation <= 2.5e-3 rad, translation direction <= 1.3e-2 rad, inlier share >= 0.988;
    3 pairs ambiguous."""
    worst, share_min, n_ambiguous = np.zeros(2), 1.0, 0
    for seed in NOISY_SEEDS:
        p = cases.make_pair(seed, 352)
        e = run(p)
        assert e["status"] == chk.OK and e["result"] == chk.SUCCESS
        share = (e["inlier"][p.truth.good] != 0).sum() / p.truth.good.sum()
        if e["ambiguous"]:
            n_ambiguous += 1
            rot, tra = best_finalist(e, p.truth)
        else:
            rot, tra = pose_errors(e["T_cur_from_ref"][:9].reshape(3, 3), e["T_cur_from_ref"][9:], p.truth)
        assert rot <= 2e-2 and tra <= 0.1 and share >= 0.9, (seed, rot, tra, share)
        worst, share_min = np.maximum(worst, [rot, tra]), min(share_min, share)
    print(f"noisy scenes: rotation {worst[0]:.1e} rad, translation direction {worst[1]:.1e} rad, inlier share {share_min:.3f}; {n_ambiguous} ambiguous")


def test_sampling_is_distinct_and_reproducible():
    for m in (4, 5, 64, 1024):
        for k in range(200):
            picks = chk.draw(3, k, m)
            assert len(set(picks)) == 4 and min(picks) >= 0 and max(picks) < m
            assert picks == chk.draw(3, k, m)
    assert sorted(chk.draw(0, 0, 4)) == [0, 1, 2, 3]
    assert chk.draw(0, 5, 100) != chk.draw(1, 5, 100)
    # every rank is drawn: over many hypotheses the picks cover a small set
    assert {r for k in range(64) for r in chk.draw(0, k, 9)} == set(range(9))


def test_degenerate_inputs():
    b = cases.batches()
    assert b["collinear"].expect[0]["status"] == chk.NO_MODEL and b["collinear"].expect[0]["best_hypothesis"] == -1
    assert b["identical_views"].expect[0]["status"] == chk.DEGENERATE and b["identical_views"].expect[0]["n_inliers_H"] == 80
    five = b["five_pairs"].expect
    assert five[1]["status"] == chk.NO_MODEL and five[3]["status"] == chk.NO_MODEL          # m = 0 and m = 3
    assert b["four_tracked"].expect[0]["result"] == chk.SUCCESS and b["four_tracked"].expect[0]["n_inliers"] == 4
    e, p = b["nan_inf_bearings"].expect[0], b["nan_inf_bearings"].pairs[0]
    idx = np.flatnonzero(p.status)
    assert e["result"] == chk.SUCCESS and not e["inlier"][idx[[3, 17, 40, 77, 99]]].any() and not e["inlier_H"][idx[[3, 17, 40, 77, 99]]].any()
    assert all(np.isfinite(e[k]).all() for k in cases.CONTINUOUS)
    e, p = b["border"].expect[0], b["border"].pairs[0]
    idx = np.flatnonzero(p.status)[:p.n_border]
    assert e["inlier"][idx].all()
    assert list(e["point_ok"][idx]) == [0, 1, 1, 0] * 4     # 9.99 out, 10.0 in, limit - 0.01 in, limit out: both views, both axes
    assert b["too_few_inliers"].expect[0]["result"] == chk.FAILURE and b["too_few_inliers"].expect[0]["status"] == chk.OK
