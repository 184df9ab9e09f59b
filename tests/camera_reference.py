"""TEST INFRASTRUCTURE, not a test.  The three camera models of the kernels (rpg_svo_amd/csrc/track_math.h) and of the C oracle
(oracle/orc_camera.h), written a third time -- from the published formulas, in mpmath at 40 digits, and NOT by translating either
of the two.  The oracle and the device header are transcriptions of one text; a slip copied into both (p1 and p2 swapped, k3 in
the wrong place of the Horner form) shows only against a derivation that does not share their lines.

Where each formula comes from:

  * pinhole: u = fx x + cx, v = fy y + cy with (x, y) = (X / Z, Y / Z) (Hartley & Zisserman, Multiple View Geometry, eq. 6.1-6.9).
  * radial-tangential ("plumb bob"): D. C. Brown, "Decentering distortion of lenses", Photogrammetric Engineering 32(3), 1966, in the
    form and coefficient order (k1 k2 p1 p2 k3) of the OpenCV calibration documentation ("Camera Calibration and 3D
    Reconstruction", the equations under "Detailed Description") and of J.-Y. Bouguet's Camera Calibration Toolbox:
        x_d = x (1 + k1 r^2 + k2 r^4 + k3 r^6) + 2 p1 x y + p2 (r^2 + 2 x^2)
        y_d = y (1 + k1 r^2 + k2 r^4 + k3 r^6) + p1 (r^2 + 2 y^2) + 2 p2 x y
    `radial` and `tangential` below are its two terms; everything else about this model is expressed through them.
  * its exact inverse: Newton's method on that forward model with the analytic Jacobian, to 1e-30.
  * OpenCV 2.4's cv::undistortPoints (what vk::PinholeCamera::cam2world calls): the fixed-point map
        x <- (x0 - tangential(x)) / radial(x)
    which follows from solving the forward model for the x in front of `radial`.  FACTS OF OPENCV AND VIKIT, which no formula
    yields (they are stated, not derived; a test can only pin that every implementation keeps them):
      - the map is iterated FIVE times (OpenCV 2.4 cvUndistortPoints: `for( j = 0; j < iters; j++ )` with iters = 5),
      - the pixel, the four intrinsics and the five coefficients are rounded to float before (vikit holds cvK_ / cvD_ as
        cv::Mat_<float> and passes a CV_32FC2 point), the arithmetic in between is double,
      - the result is rounded to float (the CV_32FC2 destination).
  * FOV / ATAN model: F. Devernay & O. Faugeras, "Straight lines have to be straight", Machine Vision and Applications 13, 2001,
    eq. (13)-(14) with omega = s:  r_d = atan(2 r tan(s / 2)) / s,  r = tan(r_d s) / (2 tan(s / 2));  s = 0 is the pinhole.
    FACTS OF VIKIT (atan_camera.{h,cpp}, inherited from PTAM's ATANCamera):
      - the constructor takes intrinsics normalised by the image size: fx_ = width fx, fy_ = height fy, cx_ = cx width - 0.5,
        cy_ = cy height - 0.5,
      - world2cam's rtrans_factor returns 1 for r < RTRANS_MIN_R, cam2world uses the factor 1 unless dist_r > INVRTRANS_MIN_R
        (the models' limits there are 2 tan(s/2) / s and its inverse, not 1: both are steps, and the product must keep them).
  * the constructor switch of vk::PinholeCamera: distortion_ = fabs(d0) > 1e-7 (FACT OF VIKIT); without it d1..d4 are ignored.
  * Reprojector::reprojectPoint (svo/src/reprojector.cpp): rigid transform, project2d, the model, `(int)` truncation toward zero,
    isInFrame(., 8), cell = (int)(v / cell_size) * n_cols + (int)(u / cell_size).  No test of the depth's sign.

Every input is a double and enters exactly (mpf(float) is exact); constants a camera struct holds rounded (1 / s, 2 tan(s / 2)) are
recomputed here from s at 40 digits, so an implementation differs from this reference by its own rounding only.

`Reference` is a class so that tests/test_camera_reference.py can judge the comparison rules with small mutants (one overridden
member each)."""
import mpmath
import numpy as np

M = mpmath.mp.clone()
M.dps = 40
mpf = M.mpf

PINHOLE, RADTAN, ATAN = 0, 1, 2          # the model tags of include/svo_hip.h
RTRANS_MIN_R = 0.001                     # FACT OF VIKIT: ATANCamera::rtrans_factor, `if(r < 0.001 || s_ == 0.0) return 1.0`
INVRTRANS_MIN_R = 0.01                   # FACT OF VIKIT: ATANCamera::cam2world, `dist_r > 0.01 ? invrtrans(dist_r) / dist_r : 1.0`
UNDISTORT_ITERATIONS = 5                 # FACT OF OPENCV 2.4: cvUndistortPoints
PINHOLE_DISTORTION_MIN_D0 = 0.0000001    # FACT OF VIKIT: PinholeCamera's distortion_(fabs(d0) > 0.0000001)
FRAME_BORDER = 8                         # reprojector.cpp: isInFrame(px.cast<int>(), 8)
INT_MIN = -2 ** 31


def f32(x):
    """x rounded to the nearest float (through the nearest double: the two roundings differ from one only for an x within 1e-16
    relative of the middle between two floats)"""
    return mpf(float(np.float32(float(x))))


class Cam:
    """a camera as svo_hip_camera / orc_pinhole hold it: model tag, size, fx fy cx cy in pixels, d = (k1 k2 p1 p2 k3) or (s, ...)"""

    def __init__(self, cam):
        self.model, self.width, self.height = int(getattr(cam, "model", PINHOLE)), int(cam.width), int(cam.height)
        self.fx, self.fy, self.cx, self.cy = (mpf(float(v)) for v in (cam.fx, cam.fy, cam.cx, cam.cy))
        self.d = tuple(mpf(float(v)) for v in getattr(cam, "d", (0.0,) * 5))
        self.s = self.d[0] if self.model == ATAN else None


def pinhole_constructor(width, height, fx, fy, cx, cy, d0, d1, d2, d3, d4):
    """-> the fields (model, fx, fy, cx, cy, d[5]) vk::PinholeCamera's constructor leaves"""
    distortion = abs(mpf(d0)) > mpf(PINHOLE_DISTORTION_MIN_D0)
    d = tuple(mpf(v) for v in (d0, d1, d2, d3, d4)) if distortion else (mpf(0),) * 5
    return (RADTAN if distortion else PINHOLE), mpf(fx), mpf(fy), mpf(cx), mpf(cy), d


def atan_constructor(width, height, fx, fy, cx, cy, s):
    """-> (model, fx_, fy_, cx_, cy_, d) with d = (s, 1 / s, 2 tan(s / 2), 1 / (2 tan(s / 2)), 0), all zero for s = 0"""
    s = mpf(s)
    d = (mpf(0),) * 5
    if s != 0:
        tans = 2 * M.tan(s / 2)
        d = (s, 1 / s, tans, 1 / tans, mpf(0))
    return ATAN, width * mpf(fx), height * mpf(fy), mpf(cx) * width - mpf("0.5"), mpf(cy) * height - mpf("0.5"), d


class Reference:
    iterations = UNDISTORT_ITERATIONS
    float_rounding = True

    # ---- Brown-Conrady ---------------------------------------------------------------------------------------------------------
    def radial(self, d, x, y):
        k1, k2, _, _, k3 = d
        r2 = x * x + y * y
        return 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3

    def tangential(self, d, x, y):
        _, _, p1, p2, _ = d
        r2 = x * x + y * y
        return 2 * p1 * x * y + p2 * (r2 + 2 * x * x), p1 * (r2 + 2 * y * y) + 2 * p2 * x * y

    def distort(self, d, x, y):
        """normalised (x, y) -> distorted normalised (x_d, y_d)"""
        rad, (tx, ty) = self.radial(d, x, y), self.tangential(d, x, y)
        return x * rad + tx, y * rad + ty

    def fixed_point(self, d, x0, y0, iterations):
        x, y = x0, y0
        for _ in range(iterations):
            rad, (tx, ty) = self.radial(d, x, y), self.tangential(d, x, y)
            x, y = (x0 - tx) / rad, (y0 - ty) / rad
        return x, y

    def undistort_exact(self, d, xd, yd):
        """the (x, y) nearest the fixed-point solution with distort(x, y) = (x_d, y_d): Newton, analytic Jacobian, to 1e-30"""
        k1, k2, p1, p2, k3 = d
        x, y = self.fixed_point(d, xd, yd, 30)
        for _ in range(60):
            fx_, fy_ = self.distort(d, x, y)
            ex, ey = fx_ - xd, fy_ - yd
            if max(abs(ex), abs(ey)) < mpf("1e-36"):
                break
            r2 = x * x + y * y
            rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
            drad = k1 + 2 * k2 * r2 + 3 * k3 * r2 ** 2          # d radial / d r^2
            a = rad + 2 * x * x * drad + 2 * p1 * y + 6 * p2 * x
            b = 2 * x * y * drad + 2 * p1 * x + 2 * p2 * y
            c = b
            e = rad + 2 * y * y * drad + 6 * p1 * y + 2 * p2 * x
            det = a * e - b * c
            x, y = x - (e * ex - b * ey) / det, y - (a * ey - c * ex) / det
        else:
            raise ArithmeticError("Newton did not converge")
        assert max(abs(v) for v in (self.distort(d, x, y)[0] - xd, self.distort(d, x, y)[1] - yd)) < mpf("1e-30")
        return x, y

    def undistort_points_opencv(self, c, u, v, iterations=None):
        """cv::undistortPoints of OpenCV 2.4 on one pixel -> normalised (x, y)"""
        r = f32 if self.float_rounding else (lambda t: t)
        fx, fy, cx, cy = r(c.fx), r(c.fy), r(c.cx), r(c.cy)
        d = tuple(r(k) for k in c.d)
        x0, y0 = (r(u) - cx) / fx, (r(v) - cy) / fy
        x, y = self.fixed_point(d, x0, y0, self.iterations if iterations is None else iterations)
        return r(x), r(y)

    # ---- Devernay-Faugeras -----------------------------------------------------------------------------------------------------
    def fov_distort_radius(self, s, r):
        return M.atan(2 * r * M.tan(s / 2)) / s

    def fov_undistort_radius(self, s, rd):
        return M.tan(rd * s) / (2 * M.tan(s / 2))

    def rtrans_is_identity(self, r):
        return r < mpf(RTRANS_MIN_R)

    def invrtrans_applies(self, dist_r):
        return dist_r > mpf(INVRTRANS_MIN_R)

    # ---- vk::AbstractCamera ----------------------------------------------------------------------------------------------------
    def world2cam_uv(self, c, x, y):
        """normalised (x, y) = project2d(xyz) -> pixel"""
        if c.model == RADTAN:
            x, y = self.distort(c.d, x, y)
        elif c.model == ATAN:
            r = M.sqrt(x * x + y * y)
            factor = mpf(1) if (self.rtrans_is_identity(r) or c.s == 0) else self.fov_distort_radius(c.s, r) / r
            x, y = factor * x, factor * y
        return c.fx * x + c.cx, c.fy * y + c.cy

    def cam2world_plane(self, c, u, v):
        """pixel -> the point (x, y) of the plane z = 1 that cam2world normalises"""
        u, v = mpf(float(u)), mpf(float(v))
        if c.model == RADTAN:
            return self.undistort_points_opencv(c, u, v)
        x, y = (u - c.cx) / c.fx, (v - c.cy) / c.fy
        if c.model == ATAN:
            dist_r = M.sqrt(x * x + y * y)
            r = dist_r if c.s == 0 else self.fov_undistort_radius(c.s, dist_r)
            factor = r / dist_r if self.invrtrans_applies(dist_r) else mpf(1)
            x, y = factor * x, factor * y
        return x, y

    def cam2world(self, c, u, v):
        """pixel -> unit bearing"""
        x, y = self.cam2world_plane(c, u, v)
        n = M.sqrt(x * x + y * y + 1)
        return x / n, y / n, 1 / n

    def exact_unproject(self, c, u, v):
        """pixel -> the (x, y) with world2cam_uv(x, y) = (u, v) on the model's own branch (no five iterations, no float, no
        threshold on this side): what the case builder uses to put a projection where it wants it"""
        x, y = (mpf(u) - c.cx) / c.fx, (mpf(v) - c.cy) / c.fy
        if c.model == RADTAN:
            return self.undistort_exact(c.d, x, y)
        if c.model == ATAN and c.s != 0:
            rd = M.sqrt(x * x + y * y)
            if rd == 0:
                return x, y
            factor = self.fov_undistort_radius(c.s, rd) / rd
            return factor * x, factor * y
        return x, y

    # ---- Reprojector::reprojectPoint -------------------------------------------------------------------------------------------
    def to_int(self, v):
        """a C cast of a finite double: toward zero; out of int's range the cast is undefined in C and INT_MIN on x86"""
        t = int(M.floor(v)) if v >= 0 else int(M.ceil(v))
        return t if -2 ** 31 <= t < 2 ** 31 else INT_MIN

    def visible(self, p):
        return True   # reprojectPoint has no test of z

    def transform(self, T, pos):
        """T [12] = (R row-major | t), pos [3] -> R pos + t"""
        T, p = [mpf(float(v)) for v in T], [mpf(float(v)) for v in pos]
        return tuple(T[3 * i] * p[0] + T[3 * i + 1] * p[1] + T[3 * i + 2] * p[2] + T[9 + i] for i in range(3))

    def reproject_point(self, c, T, pos, cell_size, n_cols):
        """-> (cell or -1, (u, v)); (u, v) is None where the point has z = 0 in the frame (the reference divides by it: inf or NaN)"""
        p = self.transform(T, pos)
        if p[2] == 0:
            return -1, None
        u, v = self.world2cam_uv(c, p[0] / p[2], p[1] / p[2])
        if not self.visible(p):
            return -1, (u, v)
        iu, iv = self.to_int(u), self.to_int(v)
        b = FRAME_BORDER
        if iu >= b and iu < c.width - b and iv >= b and iv < c.height - b:
            return self.to_int(v / cell_size) * n_cols + self.to_int(u / cell_size), (u, v)
        return -1, (u, v)


REF = Reference()


def as_double(values):
    """mpf (or None: NaN) -> the nearest doubles, as an array"""
    return np.array([np.nan if v is None else float(v) for v in values], np.float64)
