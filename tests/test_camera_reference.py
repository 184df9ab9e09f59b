"""The camera models against an independent derivation, WITHOUT a GPU.

tests/camera_reference.py restates the pinhole, the radial-tangential pinhole (with OpenCV 2.4's five-iteration inverse) and the
ATAN camera from the published formulas in mpmath; tests/camera_cases.py holds the cameras, pixels, points and the rules.  Here:
the reference is checked on its own (forward o exact inverse = identity, the ATAN pair are inverses outside vikit's two threshold
discs, the conditions on the cases), then the C oracle (oracle/orc_camera.h through orc_cam2world / orc_reproject_point), the
reference build (oracle/_ref, the shims that include orc_camera.h) and the device header compiled for the host
(rpg_svo_amd/csrc/track_math.h through hm_cam2world / hm_world2cam) are held to it under the rules, and the rules themselves are
judged with mutants of the reference -- one slip each, every one of which must be caught.

Recorded numbers (test_the_five_iteration_gap prints them; a record, not an assert beyond their order).  cv::undistortPoints'
five iterations on float-rounded input against the exact inverse, at the worst image corner, in pixels (|x - x_exact| fx):

    iterations          radtan (svo_ros/param/camera_pinhole.yaml)      radtan_k3 (k3 = -0.02, p1 = 2e-3, p2 = -1.5e-3)
        3                   3.7                                             15
        5                   0.55                                            3.5
        8                   0.032                                           0.38
       20                   4.3e-5 (the float-rounded intrinsics)           5.5e-5

The round trip cam2world -> world2cam misses the pixel by 0.54 px (radtan) and 1.4 px (radtan_k3) there: it is what the suite
knew as `< 1.0` in a comment of tests/test_device_math_host.py."""
import ctypes as C

import numpy as np
import pytest

import camera_cases as cc
import camera_reference as cr
from camera_reference import M, REF, mpf
from oracle import pytrack


# ---- the reference on its own ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.RADTAN_NAMES)
def test_forward_then_exact_inverse_is_the_identity(name):
    c = cr.Cam(cc.cameras()[name])
    rng = np.random.default_rng(1)
    x_max, y_max = float(max(c.cx, c.width - c.cx) / c.fx), float(max(c.cy, c.height - c.cy) / c.fy)
    for _ in range(40):
        # (inside the image: beyond the corners the forward model folds back and has a second preimage)
        x, y = mpf(rng.uniform(-0.9, 0.9) * x_max), mpf(rng.uniform(-0.9, 0.9) * y_max)
        xb, yb = REF.undistort_exact(c.d, *REF.distort(c.d, x, y))
        assert max(abs(xb - x), abs(yb - y)) < mpf("1e-25"), (name, x, y)


def test_textbook_form_of_the_forward_model():
    """`distort` on numbers worked by hand from the equations as printed: (k1 k2 p1 p2 k3) = (-0.3, 0.1, 0.002, -0.001, 0.05),
    x = 0.5, y = -0.25 -> r^2 = 0.3125, r^4 = 0.09765625, r^6 = 0.030517578125,
    radial = 1 - 0.09375 + 0.009765625 + 0.00152587890625 = 0.91754150390625,
    x_d = 0.458770751953125 + 2 (0.002)(-0.125) + (-0.001)(0.3125 + 0.5) = 0.457458251953125,
    y_d = -0.2293853759765625 + 0.002 (0.3125 + 0.125) + 2 (-0.001)(-0.125) = -0.2282603759765625"""
    d = tuple(mpf(v) for v in ("-0.3", "0.1", "0.002", "-0.001", "0.05"))
    x, y = mpf("0.5"), mpf("-0.25")
    assert abs(REF.radial(d, x, y) - mpf("0.91754150390625")) < mpf("1e-35")
    xd, yd = REF.distort(d, x, y)
    assert abs(xd - mpf("0.457458251953125")) < mpf("1e-35") and abs(yd - mpf("-0.2282603759765625")) < mpf("1e-35")


@pytest.mark.parametrize("name", ["atan", "atan_dyadic"])
def test_atan_pair_are_inverses_outside_the_threshold_discs(name):
    c = cr.Cam(cc.cameras()[name])
    rng = np.random.default_rng(2)
    for _ in range(60):
        r, a = mpf(10.0 ** rng.uniform(-1.9, 0.3)), mpf(rng.uniform(0, 6.28))
        x, y = r * M.cos(a), r * M.sin(a)
        u, v = REF.world2cam_uv(c, x, y)
        dist_r = M.sqrt(((u - c.cx) / c.fx) ** 2 + ((v - c.cy) / c.fy) ** 2)
        assert r >= cr.RTRANS_MIN_R and dist_r > cr.INVRTRANS_MIN_R
        # (cam2world takes doubles: undo the model by its radius functions on the unrounded pixel)
        rb = REF.fov_undistort_radius(c.s, dist_r)
        assert abs(rb - r) < mpf("1e-25") * max(1, r), (name, r)
        assert abs(REF.fov_distort_radius(c.s, rb) - dist_r) < mpf("1e-25")
    # inside the discs vikit's factor is 1 where the model's limit is 2 tan(s/2) / s = 1.079 (and 0.927 on the way back): steps
    lim = 2 * M.tan(c.s / 2) / c.s
    assert abs(REF.fov_distort_radius(c.s, mpf("1e-9")) / mpf("1e-9") - lim) < mpf("1e-15") and abs(lim - mpf("1.0793")) < mpf("1e-4")
    u_in, _ = REF.world2cam_uv(c, mpf(cr.RTRANS_MIN_R) * (1 - mpf("1e-9")), mpf(0))
    u_out, _ = REF.world2cam_uv(c, mpf(cr.RTRANS_MIN_R) * (1 + mpf("1e-9")), mpf(0))
    assert abs((u_out - u_in) - (lim - 1) * cr.RTRANS_MIN_R * c.fx) < mpf("1e-5")      # 0.030 px for the reference's yaml
    f_in = REF.cam2world_plane(c, float(c.cx) + 0.009 * float(c.fx), float(c.cy))[0] / mpf("0.009")
    f_out = REF.cam2world_plane(c, float(c.cx) + 0.011 * float(c.fx), float(c.cy))[0] / mpf("0.011")
    assert abs(f_in - 1) < mpf("1e-12") and abs(f_out - 1 / lim) < mpf("1e-3")


def test_conditions_of_the_cases():
    """the radial-tangential cameras are invertible over the image and the fixed-point map converges there; every ring is on its
    side, every point is 1e-7 px from the boundaries that decide its cell (asserted where the cases are built)"""
    for name in cc.RADTAN_NAMES:
        smallest, trips = cc.radtan_conditions(name)
        print(name, "smallest d(r radial)/dr:", smallest, "corner round trips after 5 / 10 / 20 iterations [px]:", trips)
    for name in cc.CAMERA_NAMES:
        labels, px = cc.pixels(name)
        plabels, frame, pos, exempt = cc.points(name)
        cell, _ = cc.ref_reprojections(name)
        assert len(labels) >= 77 and exempt.sum() == 2 and (cell[exempt] == -1).all()
        by = lambda word: [int(cell[i]) for i, l in enumerate(plabels) if l.startswith(word)]
        assert min(by("behind the camera, mirrored")) >= 0 and max(by("behind the camera")) >= 0    # no z test: they land in cells
        assert (cell >= 0).sum() > 40 and (cell < 0).sum() > 10
        for k in ("u = 8 ", "v = 8 "):   # the two sides of a border give two verdicts
            assert sorted(c >= 0 for c in by(k)) == [False, True], (name, k, by(k))
        for k in (f"u = {5 * cc.CELL} ", f"v = {3 * cc.CELL} "):   # the two sides of a cell boundary give two cells
            assert len(set(by(k))) == 2 and min(by(k)) >= 0, (name, k, by(k))
    # cast_int's INT_MIN path: projections beyond 2^31 px on the cameras that do not bound the image
    for name in ("pinhole", "radtan", "radtan_k3", "atan_s0"):
        plabels = cc.points(name)[0]
        _, px = cc.ref_reprojections(name)
        assert all(np.abs(px[i]).max() > 2.0 ** 31 for i, l in enumerate(plabels) if "1e7" in l)


def test_the_five_iteration_gap():
    for name in cc.RADTAN_NAMES:
        cam = cc.cameras()[name]
        c = cr.Cam(cam)
        worst = {}
        for u, v in cc._corners(cam):
            xe, ye = REF.undistort_exact(c.d, (mpf(u) - c.cx) / c.fx, (mpf(v) - c.cy) / c.fy)
            for it in (3, 5, 8, 20):
                x, y = REF.undistort_points_opencv(c, u, v, it)
                gap = float(M.sqrt(((x - xe) * c.fx) ** 2 + ((y - ye) * c.fy) ** 2))
                worst[it] = max(worst.get(it, 0.0), gap)
        print(name, "gap to the exact inverse at the worst corner [px]:", worst)
        assert worst[3] > worst[5] > worst[8] > worst[20]


# ---- the implementations against the reference -------------------------------------------------------------------------------
def _track_answers(tr, name):
    cam = cc.cameras()[name]
    f = tr.cam2world(cam, cc.pixels(name)[1])
    _, frame, pos, _ = cc.points(name)
    out = [tr.reproject_point(cam, cc.FRAMES[k], p, cc.CELL, cc.n_cols(cam)) for k, p in zip(frame, pos)]
    return f, np.array([k for k, _ in out], np.int32), np.stack([p for _, p in out])


@pytest.mark.parametrize("name", cc.CAMERA_NAMES)
def test_oracle_against_the_reference(oracle, name):
    """orc_cam2world / orc_reproject_point (oracle/orc_camera.h) on every case, under the rules"""
    cc.check_all(name, *_track_answers(pytrack.Track("orc"), name))


@pytest.mark.parametrize("name", cc.CAMERA_NAMES)
def test_reference_build_against_the_reference(name):
    """the reference's own Reprojector::reprojectPoint and Frame::c2f over the camera shims, where oracle/_ref is built"""
    if not pytrack.ref_available():
        pytest.skip("oracle/_ref/libsvo_ref.so not built (needs the reference checkout at build time)")
    cc.check_all(name, *_track_answers(pytrack.Track("ref"), name))


@pytest.fixture(scope="module")
def hm():
    import test_device_math_host as dm
    return dm._build_host_lib(dm.LIB)


@pytest.mark.parametrize("name", cc.CAMERA_NAMES)
def test_device_header_on_the_host_against_the_reference_and_the_oracle(hm, oracle, name):
    """track_math.h's cam2world / world2cam compiled for the host: under the rules against the reference, and equal to the oracle
    bit for bit on every case -- the assert of tests/test_device_math_host.py carried to where the models branch.  world2cam
    takes the point in the camera's frame: the reference's R p + t rounded to doubles (exact under the identity rotation)."""
    D = C.POINTER(C.c_double)
    p_ = lambda a: a.ctypes.data_as(D)
    cam = cc.cameras()[name]
    k, d = np.array([cam.fx, cam.fy, cam.cx, cam.cy]), np.array(cam.d, np.float64)
    orc = pytrack.Track("orc")
    _, px = cc.pixels(name)
    f = np.zeros((len(px), 3))
    for i in range(len(px)):
        hm.hm_cam2world(p_(k), cam.width, cam.height, cam.model, p_(d), p_(np.ascontiguousarray(px[i])), p_(f[i]))
    cc.check_bearings(name, f)
    assert np.array_equal(f, orc.cam2world(cam, px))
    _, frame, pos, exempt = cc.points(name)
    identity = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)
    out = np.zeros((len(pos), 2))
    for i in range(len(pos)):
        p_cam = cr.as_double(REF.transform(cc.FRAMES[frame[i]], pos[i]))
        hm.hm_world2cam(p_(k), cam.width, cam.height, cam.model, p_(d), p_(p_cam), p_(out[i]))
        _, px_o = orc.reproject_point(cam, identity, p_cam, cc.CELL, cc.n_cols(cam))
        assert np.array_equal(out[i], px_o, equal_nan=True), (name, i, out[i], px_o)
    cc.check_pixels(name, out)


# ---- the rules judged on their own -------------------------------------------------------------------------------------------
class _SwappedTangential(cr.Reference):
    def tangential(self, d, x, y):
        return super().tangential((d[0], d[1], d[3], d[2], d[4]), x, y)


class _NoK3(cr.Reference):
    def radial(self, d, x, y):
        return super().radial((d[0], d[1], d[2], d[3], 0), x, y)


class _FourIterations(cr.Reference):
    iterations = 4


class _SixIterations(cr.Reference):
    iterations = 6


class _NoFloatRounding(cr.Reference):
    float_rounding = False


class _RtransLessOrEqual(cr.Reference):
    def rtrans_is_identity(self, r):
        return r <= mpf(cr.RTRANS_MIN_R)


class _InvrtransGreaterOrEqual(cr.Reference):
    def invrtrans_applies(self, dist_r):
        return dist_r >= mpf(cr.INVRTRANS_MIN_R)


class _RoundedCell(cr.Reference):
    def to_int(self, v):
        return super().to_int(M.floor(v + mpf("0.5")))


class _DepthTest(cr.Reference):
    def visible(self, p):
        return p[2] > 0


# slip -> (the mutant, the cameras on which it is caught, the rules that catch it)
MUTANTS = {
    "p1 and p2 swapped": (_SwappedTangential, {"radtan", "radtan_k3"}, {"bearings", "pixels", "cells"}),
    "k3 dropped": (_NoK3, {"radtan_k3"}, {"bearings", "pixels", "cells"}),
    "four iterations": (_FourIterations, {"radtan", "radtan_k3"}, {"bearings"}),
    "six iterations": (_SixIterations, {"radtan", "radtan_k3"}, {"bearings"}),
    "no float rounding": (_NoFloatRounding, {"radtan", "radtan_k3"}, {"bearings"}),
    "r <= 0.001": (_RtransLessOrEqual, {"atan", "atan_dyadic"}, {"pixels"}),
    "dist_r >= 0.01": (_InvrtransGreaterOrEqual, {"atan_dyadic"}, {"bearings"}),
    "the cell rounded, not truncated": (_RoundedCell, set(cc.CAMERA_NAMES), {"cells"}),
    "a z test": (_DepthTest, set(cc.CAMERA_NAMES), {"cells"}),
}


def _caught(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def test_the_rules_accept_the_reference():
    for name in cc.CAMERA_NAMES:
        cell, px = cc.ref_reprojections(name)
        cc.check_all(name, cc.ref_bearings(name), cell, px)


@pytest.mark.parametrize("slip", list(MUTANTS))
def test_the_rules_catch(slip):
    """an answer with one slip -- the reference's own functions with one member changed -- fails a rule, on exactly the cameras
    and through exactly the rules listed above (which also says what each added camera and case is there for: k3 is caught
    by the second radial-tangential camera alone, `>=` by the one pixel at dist_r == 0.01)"""
    mutant, cameras, rules = MUTANTS[slip][0](), MUTANTS[slip][1], MUTANTS[slip][2]
    on, by = set(), set()
    for name in cc.CAMERA_NAMES:
        cell, px = cc.reprojections_of(mutant, name)
        hits = {"bearings": _caught(cc.check_bearings, name, cc.bearings_of(mutant, name)), "pixels": _caught(cc.check_pixels, name, px),
                "cells": _caught(cc.check_cells, name, cell)}
        if any(hits.values()):
            on.add(name)
        by |= {k for k, v in hits.items() if v}
    assert on == cameras and by == rules, (slip, on, by)
