"""TEST INFRASTRUCTURE, not a test.  The cases and the rules of the camera tests -- tests/test_camera_reference.py (the C oracle,
the reference build, the device header compiled for the host), tests/test_camera_edges_emulated.py (the host-emulated library)
and tests/test_camera_edges_gpu.py (the device) -- against the mpmath reference of tests/camera_reference.py.  Plain numpy,
mpmath, rpg_svo_amd.synth / se3 and helpers: nothing here touches a GPU or loads a library under test.

Cameras (CAMERAS): the three of helpers.camera_models(); the ATAN camera with s = 0; a second radial-tangential camera with
k3 != 0 and p1, p2 of opposite sign (in every other test of the suite k3 is 0 and p1 ~ p2 ~ 1e-3); and an ATAN camera with
dyadic intrinsics, on which the pixel at dist_r == 0.01 EXACTLY is representable (the only input that tells `>` from `>=`).

Pixels for cam2world (pixels): the principal point, corners, edge midpoints, pixels whose float rounding differs from the double,
64 random ones (fuzz_rng) and, for ATAN, rings around the principal point on both sides of dist_r = 0.01.

Points for reprojectPoint (points): world points under the three poses of FRAMES, built through the reference's exact inverse
so that their projections land 1e-6 px on either side of the frame border (8, size - 8) and of cell boundaries, on both sides of
the normalised radius 0.001 (ATAN) and exactly on it, at depths 0.05 / 2 / 1e4, behind the camera (reprojectPoint has no z test:
such a point is mirrored through the centre and can land in a cell), at |z| = 1e-6, at z = 0 exactly, and 64 random ones.

Conditions, asserted here where the cases are built (a case that misses one is a mistake of this file, never left out):
  * radtan_conditions: for each radial-tangential camera the radial polynomial's derivative is positive out to the undistorted
    radius of every image corner, and the round-trip error of the fixed-point map decreases from 5 to 10 to 20 iterations there.
  * every ring is on the side of its threshold it was built for, by at least 5e-10 relative (a double evaluation of the radius
    is within a few 1e-16).
  * every point's reference pixel is at least 1e-7 px from every boundary that decides its cell (1000 x the pixel rule), so the
    cell is exact on every backend.  The z = 0 points are exempt: the reference's `(int)` of inf / NaN is undefined C; the rule
    for them is only cell == -1.

Why three poses: the pixel rule is relative 1e-13.  R p + t in doubles carries an ABSOLUTE error of ~1e-16 times the size of
its terms, so a camera-frame depth of 1e-6 formed from terms of size 1 is good to 1e-10 relative -- no double implementation
could meet the rule there, the reference's included.  The |z| = 1e-6 points therefore sit under a pose whose translation is of
their own size (FRAMES[1], a generic rotation) or under the pose with the identity rotation (FRAMES[2]), where R p + t is exact;
the z = 0 and r == 0.001 points need that exactness too.

Rules: check_bearings (1e-12, the bound of tests/test_device_math_host.py for math that is not bit-exact; a float ulp of the
radial-tangential result is 6e-8, so a wrong rounding cannot hide), check_pixels (1e-10 + 1e-13 |px_ref|: check_reproject_points'
1e-10 with a relative term for far-away projections), check_cells (identical), check_constructor."""
import functools
import math

import numpy as np

import camera_reference as cr
from camera_reference import M, REF, mpf
from helpers import camera_models, fuzz_rng
from rpg_svo_amd import se3, synth

CELL = 30
BEARING_TOL = 1e-12
PIXEL_ATOL, PIXEL_RTOL = 1e-10, 1e-13
CELL_MARGIN = 1e-7
SIDE_MARGIN = 5e-10

_ATAN_YAML = (752, 480, 0.509326, 0.796651, 0.45905, 0.510056)


def _atan_dyadic():
    c = synth.Camera.atan(752, 480, 1.0, 1.0, 0.0, 0.0, 0.9320)
    return synth.Camera(752, 480, 512.0, 256.0, 2.5, 240.0, synth.CAM_ATAN, c.d)


@functools.lru_cache(None)
def cameras():
    """name -> synth.Camera"""
    cams = dict(camera_models())
    cams["atan_s0"] = synth.Camera.atan(*_ATAN_YAML, 0.0)
    cams["radtan_k3"] = synth.Camera.radtan(752, 480, 600.0, 598.0, 370.0, 236.0, -0.35, 0.12, 2e-3, -1.5e-3, -0.02)
    cams["atan_dyadic"] = _atan_dyadic()
    return cams


CAMERA_NAMES = ("pinhole", "radtan", "atan", "atan_s0", "radtan_k3", "atan_dyadic")
RADTAN_NAMES = ("radtan", "radtan_k3")


def n_cols(cam):
    return -(-cam.width // CELL)


def _corners(cam):
    return [(0.0, 0.0), (float(cam.width), 0.0), (0.0, float(cam.height)), (float(cam.width), float(cam.height))]


# ---- conditions on the radial-tangential cameras -----------------------------------------------------------------------------
@functools.lru_cache(None)
def radtan_conditions(name):
    """-> (smallest d(r radial(r)) / dr up to the corners' undistorted radius, per corner the round-trip error in px after
    5, 10 and 20 iterations of the fixed-point map in exact arithmetic); asserts the two conditions of this file's docstring"""
    cam = cameras()[name]
    c = cr.Cam(cam)
    k1, k2, _, _, k3 = c.d
    deriv = lambda r: 1 + 3 * k1 * r ** 2 + 5 * k2 * r ** 4 + 7 * k3 * r ** 6
    smallest, trips = mpf(1), []
    for u, v in _corners(cam):
        xd, yd = (mpf(u) - c.cx) / c.fx, (mpf(v) - c.cy) / c.fy
        x, y = REF.undistort_exact(c.d, xd, yd)
        r_corner = M.sqrt(x * x + y * y)
        smallest = min([smallest] + [deriv(r_corner * k / 200) for k in range(201)])
        err = []
        for it in (5, 10, 20):
            xi, yi = REF.fixed_point(c.d, xd, yd, it)
            ub, vb = REF.world2cam_uv(c, xi, yi)
            err.append(float(M.sqrt((ub - u) ** 2 + (vb - v) ** 2)))
        assert err[0] > err[1] > err[2], (name, u, v, err)
        trips.append(tuple(err))
    assert smallest > 0, (name, smallest)
    return float(smallest), trips


# ---- pixels for cam2world ----------------------------------------------------------------------------------------------------
def _ring(cam, rho_x, rho_y, n=8, phase=0.3):
    return [(cam.cx + rho_x * math.cos(phase + 2 * math.pi * k / n), cam.cy + rho_y * math.sin(phase + 2 * math.pi * k / n)) for k in range(n)]


@functools.lru_cache(None)
def pixels(name):
    """-> (labels [n], px [n,2] f64)"""
    cam = cameras()[name]
    w, h = float(cam.width), float(cam.height)
    L = [("principal point", (cam.cx, cam.cy))]
    L += [("corner", p) for p in _corners(cam)]
    L += [("edge midpoint", p) for p in ((w / 2, 0.0), (w / 2, h), (0.0, h / 2), (w, h / 2))]
    L += [("float != double", p) for p in ((751.99999, 0.1), (0.1, 479.99999), (123.456789012345, 321.987654321), (cam.cx + 1e-9, cam.cy - 1e-9))]
    rng = fuzz_rng(401)
    L += [("random", (rng.uniform(0, w), rng.uniform(0, h))) for _ in range(64)]
    if cam.model == synth.CAM_ATAN:
        c = cr.Cam(cam)
        for rel in (-1e-9, 1e-9, -1e-3, 1e-3):
            rho = cr.INVRTRANS_MIN_R * (1 + rel)
            for p in _ring(cam, rho * cam.fx, rho * cam.fy):
                dist_r = M.sqrt(((mpf(p[0]) - c.cx) / c.fx) ** 2 + ((mpf(p[1]) - c.cy) / c.fy) ** 2)
                side = dist_r / mpf(cr.INVRTRANS_MIN_R) - 1
                assert side * rel > 0 and abs(side) >= SIDE_MARGIN, (name, rel, p, side)
                L.append((f"dist_r = 0.01 (1 {rel:+g})", p))
        for radius in (0.1, 1.0, 3.0):
            L += [(f"{radius} px from the principal point", p) for p in _ring(cam, radius, radius)]
    if name == "atan_dyadic":
        c = cr.Cam(cam)
        for sign in (1.0, -1.0):
            p = (cam.cx + sign * cr.INVRTRANS_MIN_R * cam.fx, cam.cy)
            assert abs((mpf(p[0]) - c.cx) / c.fx) == mpf(cr.INVRTRANS_MIN_R), p   # exactly the threshold, in exact arithmetic
            L.append(("dist_r == 0.01", p))
    return [l for l, _ in L], np.array([p for _, p in L], np.float64)


# ---- points for reprojectPoint -----------------------------------------------------------------------------------------------
def _frames():
    generic = se3.exp(np.array([0.4, -0.3, 0.6, 0.2, -0.3, 0.25]))
    near = se3.join(se3.split(se3.exp(np.array([0.0, 0.0, 0.0, -0.3, 0.2, 0.4])))[0], np.array([2e-6, -1e-6, 1.5e-6]))
    aligned = se3.join(np.eye(3), np.array([0.0, 0.0, 1.0]))
    return np.ascontiguousarray(np.stack([generic, near, aligned]), dtype=np.float64)


FRAMES = _frames()   # T_f_w [3,12]: a generic pose; a generic rotation with a translation of 1e-6; identity rotation, t = (0, 0, 1)
GENERIC, NEAR, ALIGNED = 0, 1, 2


def _to_world(frame, p_cam):
    """R^T (p_cam - t) at 40 digits, rounded to doubles"""
    T = [mpf(float(v)) for v in FRAMES[frame]]
    q = [mpf(p_cam[i]) - T[9 + i] for i in range(3)]
    return tuple(float(T[i] * q[0] + T[3 + i] * q[1] + T[6 + i] * q[2]) for i in range(3))


def _place(c, frame, u, v, z):
    """the world point whose camera-frame depth is z and whose projection is the pixel (u, v) (for z < 0: mirrored into it)"""
    x, y = REF.exact_unproject(c, u, v)
    return _to_world(frame, (x * z, y * z, mpf(z)))


@functools.lru_cache(None)
def points(name):
    """-> (labels [n], frame [n] i32, pos [n,3] f64, exempt [n] bool: the z = 0 points)"""
    cam = cameras()[name]
    c = cr.Cam(cam)
    w, h = cam.width, cam.height
    L = []
    add = lambda label, frame, pos: L.append((label, frame, pos))
    for eps in (-1e-6, 1e-6):
        for k in (8, w - 8, 5 * CELL, 17 * CELL):
            add(f"u = {k} {eps:+g}", GENERIC, _place(c, GENERIC, k + eps, 143.7, 2.0))
        for k in (8, h - 8, 3 * CELL, 11 * CELL):
            add(f"v = {k} {eps:+g}", GENERIC, _place(c, GENERIC, 217.3, k + eps, 2.0))
    if cam.model == synth.CAM_ATAN:
        for rel in (-1e-9, 1e-9, -1e-3, 1e-3):
            rho = cr.RTRANS_MIN_R * (1 + rel)
            for k in range(8):
                a = 0.3 + 2 * math.pi * k / 8
                add(f"r = 0.001 (1 {rel:+g})", GENERIC, _to_world(GENERIC, (2 * rho * math.cos(a), 2 * rho * math.sin(a), 2.0)))
        add("r == 0.001", ALIGNED, (cr.RTRANS_MIN_R, 0.0, 0.0))
        add("r == 0.001", ALIGNED, (0.0, -2 * cr.RTRANS_MIN_R, 1.0))
    for z in (0.05, 2.0, 1e4):
        for u, v in ((100.3, 50.7), (600.4, 400.2), (cam.cx + 20.3, cam.cy - 10.7)):
            add(f"depth {z:g}", GENERIC, _place(c, GENERIC, u, v, z))
    for u, v in ((200.2, 100.6), (500.9, 300.1)):
        add("behind the camera, mirrored into the frame", GENERIC, _place(c, GENERIC, u, v, -2.0))
    for p in ((3.0, 1.0, -2.0), (-0.2, 4.0, -2.0)):
        add("behind the camera", GENERIC, _to_world(GENERIC, p))
    for z in (1e-6, -1e-6):
        for u, v in ((300.3, 200.8), (50.2, 400.6)):
            add(f"z = {z:g}", NEAR, _place(c, NEAR, u, v, z))
        add(f"z = {z:g}", NEAR, _to_world(NEAR, (5e-6, -2e-6, z)))
        add(f"z = {z:g}, |uv| ~ 1e7", ALIGNED, (8.0, -6.0, -1.0 + z))
    add("z = 0", ALIGNED, (0.5, 0.25, -1.0))
    add("z = 0, x = y = 0", ALIGNED, (0.0, 0.0, -1.0))
    rng = fuzz_rng(402)
    ex, ey = 0.7 * max(cam.cx, w - cam.cx) / cam.fx, 0.7 * max(cam.cy, h - cam.cy) / cam.fy
    for _ in range(64):
        z = rng.uniform(0.5, 20.0)
        add("random", GENERIC, _to_world(GENERIC, (z * rng.uniform(-1.4 * ex, 1.4 * ex), z * rng.uniform(-1.4 * ey, 1.4 * ey), z)))
    labels, frame, pos = [l for l, _, _ in L], np.array([f for _, f, _ in L], np.int32), np.array([p for _, _, p in L], np.float64)
    exempt = np.array([l.startswith("z = 0") for l in labels])
    _assert_point_conditions(name, labels, frame, pos, exempt)
    return labels, frame, pos, exempt


def _assert_point_conditions(name, labels, frame, pos, exempt):
    cam = cameras()[name]
    c = cr.Cam(cam)
    for i, label in enumerate(labels):
        p = REF.transform(FRAMES[frame[i]], pos[i])
        if exempt[i]:
            assert p[2] == 0, (name, label, p)
            continue
        assert p[2] != 0, (name, label)
        if label.startswith("r = 0.001"):
            rel = float(label[label.index("(1 ") + 3:-1])
            side = M.sqrt(p[0] ** 2 + p[1] ** 2) / abs(p[2]) / mpf(cr.RTRANS_MIN_R) - 1
            assert side * rel > 0 and abs(side) >= SIDE_MARGIN, (name, label, side)
        if label == "r == 0.001":
            assert M.sqrt(p[0] ** 2 + p[1] ** 2) / abs(p[2]) == mpf(cr.RTRANS_MIN_R), (name, label)
        cell, (u, v) = REF.reproject_point(c, FRAMES[frame[i]], pos[i], CELL, n_cols(cam))
        assert _cell_margin(cam, cell, u, v) >= CELL_MARGIN, (name, i, label, float(u), float(v))


def _cell_margin(cam, cell, u, v):
    """the distance in px of the reference pixel from the nearest boundary that decides its cell: in the frame, the four borders
    and the cell boundaries around it; outside, the border it violates by the most (one violated border decides -1)"""
    lo, hi_u, hi_v = cr.FRAME_BORDER, cam.width - cr.FRAME_BORDER, cam.height - cr.FRAME_BORDER
    if cell >= 0:
        inside = [u - lo, hi_u - u, v - lo, hi_v - v]
        grid = [t - CELL * M.floor(t / CELL) for t in (u, v)]
        return float(min(inside + grid + [CELL - g for g in grid]))
    return float(max(lo - u, u - hi_u, lo - v, v - hi_v))


# ---- the reference's answers (any Reference: the mutants of tests/test_camera_reference.py go through here too) --------------------
def bearings_of(model, name):
    c, (_, px) = cr.Cam(cameras()[name]), pixels(name)
    return np.stack([cr.as_double(model.cam2world(c, u, v)) for u, v in px])


def reprojections_of(model, name):
    """-> cell [n] i32, px [n,2] f64 (NaN for the z = 0 points)"""
    cam = cameras()[name]
    c, (_, frame, pos, _) = cr.Cam(cam), points(name)
    out = [model.reproject_point(c, FRAMES[f], p, CELL, n_cols(cam)) for f, p in zip(frame, pos)]
    return np.array([k for k, _ in out], np.int32), np.stack([cr.as_double(p if p is not None else (None, None)) for _, p in out])


@functools.lru_cache(None)
def ref_bearings(name):
    return bearings_of(REF, name)


@functools.lru_cache(None)
def ref_reprojections(name):
    return reprojections_of(REF, name)


# ---- rules -------------------------------------------------------------------------------------------------------------------
def check_bearings(name, f):
    f_ref, (labels, _) = ref_bearings(name), pixels(name)
    err = np.abs(np.asarray(f, np.float64).reshape(f_ref.shape) - f_ref).max(axis=1)
    bad = np.flatnonzero(~(err <= BEARING_TOL))
    assert bad.size == 0, (name, [(labels[i], err[i]) for i in bad[:5]])
    return float(err.max())


def check_pixels(name, px):
    (_, px_ref), (labels, _, _, exempt) = ref_reprojections(name), points(name)
    px = np.asarray(px, np.float64).reshape(px_ref.shape)
    with np.errstate(invalid="ignore"):
        err = np.abs(px - px_ref)
        ok = (err <= PIXEL_ATOL + PIXEL_RTOL * np.abs(px_ref)).all(axis=1) | exempt
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (name, [(labels[i], px[i], px_ref[i]) for i in bad[:5]])
    return float(np.nanmax(np.where(exempt[:, None], 0.0, err / (PIXEL_ATOL + PIXEL_RTOL * np.abs(px_ref)))))   # the largest share of the bound used


def check_cells(name, cell):
    (cell_ref, _), (labels, _, _, _) = ref_reprojections(name), points(name)
    cell = np.asarray(cell).reshape(cell_ref.shape)
    bad = np.flatnonzero(cell != cell_ref)
    assert bad.size == 0, (name, [(labels[i], int(cell[i]), int(cell_ref[i])) for i in bad[:5]])


def check_all(name, f, cell, px):
    check_bearings(name, f)
    check_pixels(name, px)
    check_cells(name, cell)


# ---- constructors ------------------------------------------------------------------------------------------------------------
PINHOLE_CTOR_ARGS = [(752, 480, 414.536145, 414.284429, 348.804988, 240.076451, d0, 0.066674, 0.000896, -0.000778, 0.013)
                     for d0 in (0.0, 9e-8, 1e-7, 1.1e-7, -1.1e-7)]
ATAN_CTOR_ARGS = [(*_ATAN_YAML, s) for s in (0.0, 0.9320)]
# a field is at most three operations, each rounded correctly or (tan) to an ulp, away from the exact value: 4 ulp
CTOR_RTOL = 4 * 2.0 ** -52


def check_constructor(kind, args, got):
    """got: an object with model, width, height, fx, fy, cx, cy, d (svo_hip_camera, orc_pinhole).  pinhole: every field a copy
    (identical), d1..d4 zero with d0 where fabs(d0) > 1e-7 is false; ATAN: the normalisation and the four constants to 4 ulp, all
    five zero for s == 0."""
    model, fx, fy, cx, cy, d = (cr.pinhole_constructor if kind == "pinhole" else cr.atan_constructor)(*args)
    assert (int(got.model), int(got.width), int(got.height)) == (model, args[0], args[1]), (kind, args, got.model)
    for what, g, want in [("fx", got.fx, fx), ("fy", got.fy, fy), ("cx", got.cx, cx), ("cy", got.cy, cy)] + [(f"d{i}", got.d[i], d[i]) for i in range(5)]:
        want = float(want)
        tol = 0.0 if (kind == "pinhole" or want == 0.0) else CTOR_RTOL * abs(want)
        assert abs(float(g) - want) <= tol, (kind, args, what, float(g), want)
