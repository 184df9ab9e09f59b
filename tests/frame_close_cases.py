"""TEST INFRASTRUCTURE.  The cases of the K11 tests (numpy only): what svo_hip_select_matches and svo_hip_pose_optimize leave
for B sequences, built by hand so that every rule of svo_hip_frame_close (include/svo_hip.h) is exercised on the smallest
shapes at which it can go wrong, and the checker's answer per batch (tests/frame_close_checker.py, computed once per process).

Rows without a point carry NaN positions and NaN bearings; rows beyond n carry has_point = 1, NaN everywhere and pixels of
-777; keyframes beyond n_kf carry NaN poses and overlap 0: nothing of theirs may be read.  Poses are random rotations of up to
3 rad, so all four branches of the quaternion conversion occur.  The comparison rules are K10's
(host_buffers.compare_bits for the emulation, first_map_cases.compare_device for the GPU: discrete outputs equal, f64 within 1e-14 relative -- the values
are K10's chains of under ten IEEE operations)."""
import functools
import types

import numpy as np

import frame_close_checker as chk
from first_map_cases import CAMERAS, bearing, grid
from homography_cases import rodrigues

INPUTS = ("n", "px", "f", "pos", "has_point", "T_f_w", "T_last", "num_obs", "num_obs_last", "n_kf", "kf_T", "kf_overlap")
DISCRETE = ("gate", "quality", "result", "nobs_out", "kf_block", "valid", "key_pts", "occupancy", "kf_remove")
CONTINUOUS = ("T_out", "depth_mean", "depth_min", "xyz_ref")
IDENTITY = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])


def pose(rng, identity=False, angle=3.0):
    axis = rng.normal(size=3)
    R = np.eye(3) if identity else rodrigues(axis / np.linalg.norm(axis) * rng.uniform(0.0, angle))
    return np.concatenate([R.reshape(9), rng.uniform(-1, 1, 3)])


def point_mask(n, mode):
    m = np.zeros(n, np.uint8)
    if mode == "all":
        m[:] = 1
    elif mode == "alternating":
        m[::2] = 1
    elif mode == "first" and n:
        m[0] = 1
    elif mode == "last" and n:
        m[-1] = 1
    elif mode == "random":
        m[:] = np.random.default_rng(n).uniform(size=n) < 0.7
    return m            # ("none": all 0)


def make_seq(cam, seed, n_stride, n, points="random", n_kf=2, kf_stride=4, overlap="all", num_obs=60, num_obs_last=70, identity=False,
             kf_spread=0.5):
    """n rows (n may exceed n_stride: the entry clamps) with random pixels inside the image, the points in front of the frame;
    n_kf keyframes around the frame's position"""
    rng = np.random.default_rng(seed)
    rows = min(max(n, 0), n_stride)
    s = types.SimpleNamespace(cam=cam, n_stride=n_stride, kf_stride=kf_stride, n=np.int32(n), num_obs=np.int32(num_obs),
                              num_obs_last=np.int32(num_obs_last), n_kf=np.int32(n_kf))
    s.has_point = np.ones(n_stride, np.uint8)
    s.has_point[:rows] = point_mask(rows, points)
    s.px = np.full((n_stride, 2), -777.0)
    s.px[:rows] = np.stack([rng.uniform(0, cam.width - 1, rows), rng.uniform(0, cam.height - 1, rows)], axis=1)
    s.T_f_w, s.T_last = pose(rng, identity), pose(rng)
    R, t = s.T_f_w[:9].reshape(3, 3), s.T_f_w[9:]
    on = np.flatnonzero(s.has_point[:rows])
    s.f, s.pos = np.full((n_stride, 3), np.nan), np.full((n_stride, 3), np.nan)
    s.f[on] = bearing(cam, s.px[on])
    s.pos[on] = (s.f[on] * rng.uniform(0.5, 4.0, (len(on), 1)) - t) @ R      # R' (x - t)
    live = min(max(n_kf, 0), kf_stride)
    s.kf_T = np.full((kf_stride, 12), np.nan)
    centre = -R.T @ t
    for i in range(live):
        T = pose(rng, angle=1.0)
        Rk = T[:9].reshape(3, 3)
        T[9:] = -Rk @ (centre + rng.normal(size=3) * kf_spread * rng.uniform(0.0, 1.0))
        s.kf_T[i] = T
    s.kf_overlap = np.zeros(kf_stride, np.int32)
    s.kf_overlap[:live] = {"all": np.arange(live), "none": -1, "one": -1}[overlap]
    if overlap == "one" and live:
        s.kf_overlap[live // 2] = 0
    return s


def set_rows(s, rows, pixels, with_bearing=True):
    rows = np.asarray(rows)
    s.px[rows] = np.asarray(pixels, np.float64)
    if with_bearing:
        on = rows[s.has_point[rows] != 0]
        s.f[on] = bearing(s.cam, s.px[on])


def on_the_centre_lines(cam, seed):
    """rows exactly on cu, on cv and on px[0] == cv; rows in no quadrant and in two; the image centre itself twice"""
    s = make_seq(cam, seed, 70, 66, points="random")
    cu, cv = cam.width // 2, cam.height // 2
    between = (min(cu, cv) + max(cu, cv)) / 2.0
    special = [(cu, cv), (cu, cv), (cu, 1.0), (cu, cam.height - 2.0), (1.0, cv), (cam.width - 2.0, cv), (cv, cv), (cv, 2.0), (cv, cam.height - 3.0),
               (between, 3.0), (between, cam.height - 3.0), (cu - 0.5, cv - 0.5), (cu + 0.5, cv - 0.5), (cu - 0.5, cv + 0.5), (cu + 0.5, cv + 0.5)]
    rows = np.flatnonzero(s.has_point[:66])[3:3 + len(special)]
    set_rows(s, rows, special)
    s.centre_row = int(rows[0])
    return s


def only_between(cam, seed):
    """every row has lo <= px[0] < hi (lo, hi = cv, cu in either order)"""
    s = make_seq(cam, seed, 20, 16, points="alternating")
    cu, cv = cam.width // 2, cam.height // 2
    rng = np.random.default_rng(seed + 1)
    set_rows(s, np.arange(16), np.stack([rng.uniform(min(cu, cv), max(cu, cv) - 0.01, 16), rng.uniform(0, cam.height - 1, 16)], axis=1))
    return s


def duplicated_pixels(cam, seed):
    """the second half of the rows repeats the pixels of the first half in reverse order: a tie for every key point"""
    s = make_seq(cam, seed, 130, 100, points="all")
    s.px[50:100] = s.px[:50][::-1]
    s.f[50:100] = s.f[:50][::-1]
    return s


def bad_pixels(cam, seed, cell_size, nan_first):
    """rows whose pixel is NaN, infinite, negative by more than a cell, beyond the grid or huge, with and without a point; a
    NaN pixel on the first row with a point (it stays key point 0) or only on later ones"""
    s = make_seq(cam, seed, 40, 36, points="alternating")
    _, n_cols, n_rows = grid(cam, cell_size)
    bad = [(np.nan, 5.0), (5.0, np.nan), (np.inf, 5.0), (5.0, -np.inf), (-cell_size - 1.0, 5.0), (5.0, -2.0 * cell_size), (n_cols * cell_size, 5.0),
           (5.0, n_rows * cell_size), (1e30, 5.0), (5.0, -1e30), (3e9, 3e9), (-0.5 * cell_size, 5.0), (n_cols * cell_size - 0.25, n_rows * cell_size - 0.25)]
    set_rows(s, np.arange(3, 3 + len(bad)), bad, with_bearing=False)      # rows 3 .. 15: odd ones have no point
    set_rows(s, [20], [(np.nan, np.nan)], with_bearing=False)
    if nan_first:
        set_rows(s, [0], [(np.nan, 3.0)], with_bearing=False)
    s.n_bad = len(bad)
    return s


def equal_depths(cam, seed, n_points):
    """identity pose; five points around the median rank share one depth, and so do the two smallest; holes between them"""
    n = 2 * n_points + 3
    s = make_seq(cam, seed, n + 4, n, points="alternating", identity=True)
    s.T_f_w[9:] = (0.0, 0.0, 0.25)
    on = np.flatnonzero(s.has_point[:n])[:n_points]
    s.has_point[:n] = 0
    s.has_point[on] = 1
    z = np.random.default_rng(seed).uniform(1.0, 4.0, n_points)
    order = np.argsort(z)
    mid = n_points // 2
    z[order[max(mid - 2, 0):mid + 3]] = z[order[mid]]
    if n_points > 1:
        z[order[1]] = z[order[0]]
    s.pos[:] = np.nan
    s.pos[on] = s.f[on] * 2.0
    s.pos[on, 2] = z
    s.z_cam = z + 0.25
    return s


def kf_box(cam, axis, value, others=0.0):
    """identity poses, every point at depth 2 (depth_mean = 2, a power of two), one overlapping keyframe whose position is
    `value` on `axis` and `others` elsewhere: relpos = kf_pos exactly"""
    s = make_seq(cam, 5, 12, 10, points="all", n_kf=1, kf_stride=2, identity=True)
    s.T_f_w = IDENTITY.copy()
    s.pos[:10] = s.f[:10] / s.f[:10, 2:3] * 2.0
    s.pos[:10, 2] = 2.0
    T = IDENTITY.copy()
    p = np.full(3, others)
    p[axis] = value
    T[9:] = -p
    s.kf_T[0] = T
    return s


def far_kfs(cam, positions, n=10):
    """identity poses, the frame at the origin, keyframes at the given positions (none overlaps)"""
    k = len(positions)
    s = make_seq(cam, 6, 12, n, points="all", n_kf=k, kf_stride=8, overlap="none", identity=True)
    s.T_f_w = IDENTITY.copy()
    for i, p in enumerate(positions):
        s.kf_T[i] = IDENTITY
        s.kf_T[i, 9:] = -np.asarray(p, np.float64)
    return s


def _batch(name, seqs, cell_size, params=None):
    cam = seqs[0].cam
    assert len({(s.n_stride, s.kf_stride) for s in seqs}) == 1 and all(s.cam is cam for s in seqs)
    return types.SimpleNamespace(name=name, seqs=seqs, cam=cam, n_stride=seqs[0].n_stride, kf_stride=seqs[0].kf_stride, grid=grid(cam, cell_size),
                                 params=dict(params or {}))


MODES = ("none", "all", "alternating", "first", "last", "random")
EQUAL_DEPTH_COUNTS = (1, 2, 5, 6, 31, 32)
BOX = dict(kfselect_mindist=0.125, quality_min_fts=5, min_pose_obs=5)   # depth_mean = 2: |x| < 0.25, |y| < 2 (0.125 * 0.8), |z| < 2 (0.125 * 1.3)
BOX_BOUNDS = (0.25, 2.0 * (0.125 * 0.8), 2.0 * (0.125 * 1.3))


@functools.lru_cache(maxsize=None)
def batches():
    """name -> batch, with the checker's answer as .expect.  (Built once per process; the tests never write the arrays.)"""
    out = []
    wide, odd, tiny, tall = (CAMERAS[k] for k in ("160x120", "150x118", "47x33", "33x47"))
    # sizes around the strides of the loops and around quality_min_fts; n beyond the stride is clamped
    for (cam, cell), n_stride, ns in ((tiny, 1, (0, 1, 5)), (wide, 65, (0, 1, 49, 50, 63, 64, 65, 70)), (odd, 257, (121, 255, 256, 257, 300)),
                                      (wide, 1024, (1024, 2000, 121))):
        out.append(_batch(f"rows{n_stride}", [make_seq(cam, 1000 * n_stride + k, n_stride, n, points=MODES[(k + 1) % 6], num_obs=min(max(n, 0), 60),
                                                       num_obs_last=60) for k, n in enumerate(ns)], cell))
    out.append(_batch("point_modes", [make_seq(wide[0], 70 + k, 70, 66, points=m) for k, m in enumerate(MODES)], wide[1]))
    for n in EQUAL_DEPTH_COUNTS:
        out.append(_batch(f"equal_depths_{n}", [equal_depths(odd[0], 20 + n, n)], odd[1], dict(quality_min_fts=1)))
    # the keyframe list: sizes around max_n_kfs and the stride, none / one / all of them overlapping
    out.append(_batch("keyframes", [make_seq(wide[0], 300 + 7 * k + j, 60, 55, n_kf=n_kf, kf_stride=64, overlap=ov, kf_spread=(0.1, 0.5, 2.0)[j])
                                    for k, n_kf in enumerate((0, 1, 9, 10, 11, 64, 70)) for j, ov in enumerate(("none", "one", "all"))], wide[1]))
    for key, (cam, cell) in CAMERAS.items():
        out.append(_batch(f"centre_lines_{key}", [on_the_centre_lines(cam, 7), on_the_centre_lines(cam, 9)], cell))
        out.append(_batch(f"between_{key}", [only_between(cam, 8)], cell))
        out.append(_batch(f"ties_{key}", [duplicated_pixels(cam, 11)], cell))
        out.append(_batch(f"bad_pixels_{key}", [bad_pixels(cam, 51, cell, True), bad_pixels(cam, 52, cell, False)], cell))
    # every gate, one off either side (default parameters): (n, num_obs, num_obs_last)
    gates = ((49, 60, 60), (50, 60, 60), (60, 19, 30), (60, 20, 30), (60, 50, 90), (60, 50, 91), (121, 80, 200), (121, 79, 200), (60, 49, 49),
             (60, 50, 50))
    out.append(_batch("gates", [make_seq(wide[0], 400 + k, 121, n, points="all", num_obs=a, num_obs_last=b) for k, (n, a, b) in enumerate(gates)],
                      wide[1]))
    # quality_min_fts 10, so that 20 observations pass the second gate and the third
    low = ((9, 30, 30), (10, 30, 30), (60, 19, 30), (60, 20, 30), (60, 9, 9))
    out.append(_batch("gates_low_min", [make_seq(wide[0], 420 + k, 70, n, points="all", num_obs=a, num_obs_last=b) for k, (n, a, b) in enumerate(low)],
                      wide[1], dict(quality_min_fts=10)))
    # needNewKf: each axis exactly on its bound, just inside and just outside, the other two axes at 0 and just inside
    box = []
    for axis, bound in enumerate(BOX_BOUNDS):
        for value in (bound, np.nextafter(bound, 0.0), np.nextafter(bound, 9.0), -bound, -np.nextafter(bound, 0.0)):
            box.append(kf_box(wide[0], axis, value))
        box.append(kf_box(wide[0], axis, np.nextafter(bound, 0.0), others=np.nextafter(BOX_BOUNDS[0], 0.0) / 2))
    out.append(_batch("kf_box", box, wide[1], BOX))
    # getFurthestKeyframe: a tie between two and between three, all distances 0; max_n_kfs 3 (n_kf 2, 3, 4) and 2
    P = [(0, 0, 1.0), (0.5, 0, 0), (0, 0, -1.0), (0, 1.0, 0)]
    far = [far_kfs(wide[0], P[:2]), far_kfs(wide[0], P[:3]), far_kfs(wide[0], P), far_kfs(wide[0], [(0, 0, 0)] * 3),
           far_kfs(wide[0], [(0, 0, 0), (3.0, 4.0, 0), (0, 5.0, 0), (5.0, 0, 0)])]
    out.append(_batch("furthest_3", far, wide[1], dict(max_n_kfs=3, quality_min_fts=5)))
    out.append(_batch("furthest_2", far, wide[1], dict(max_n_kfs=2, quality_min_fts=5)))
    # adjacent sequences leave by every exit; 0 and 5 are identical, and so are 2 and 7 (sixteen sequences: the XCD-contiguous
    # workgroup order is a permutation there)
    def exits(k):
        kind = k % 5
        seed = 500 + kind
        if kind == 0:
            return make_seq(wide[0], seed, 121, 70, num_obs=60, num_obs_last=70, n_kf=3, kf_spread=3.0, overlap="none")   # IS_KEYFRAME
        if kind == 1:
            return make_seq(wide[0], seed, 121, 30)                                                                      # gate 1
        if kind == 2:
            return make_seq(wide[0], seed, 121, 70, num_obs=10)                                                          # gate 2
        if kind == 3:
            return make_seq(wide[0], seed, 121, 121, num_obs=55, num_obs_last=110)                                       # gate 3
        return make_seq(wide[0], seed, 121, 70, n_kf=3, kf_spread=0.0)                                                   # NO_KEYFRAME
    out.append(_batch("every_exit", [exits(k) for k in range(16)], wide[1]))
    out = {b.name: b for b in out}
    for b in out.values():
        b.expect = chk.frame_close(b.cam, inputs(b), *b.grid, params=b.params)
    return out


def _names():
    n = ["rows1", "rows65", "rows257", "rows1024", "point_modes", "keyframes", "gates", "gates_low_min", "kf_box", "furthest_3", "furthest_2", "every_exit"]
    for key in ("160x120", "150x118", "47x33", "33x47"):
        n += [f"centre_lines_{key}", f"between_{key}", f"ties_{key}", f"bad_pixels_{key}"]
    return tuple(n + [f"equal_depths_{k}" for k in EQUAL_DEPTH_COUNTS])


NAMES = _names()


def inputs(b):
    """the arrays of a batch as the entry takes them, by name"""
    dt = dict(n=np.int32, has_point=np.uint8, num_obs=np.int32, num_obs_last=np.int32, n_kf=np.int32, kf_overlap=np.int32)
    return {k: np.ascontiguousarray(np.stack([getattr(s, k) for s in b.seqs]), dtype=dt.get(k, np.float64)) for k in INPUTS}


def out_shapes(B, n_stride, cells):
    """name -> (shape, dtype) of svo_hip_frame_close_out, in the struct's order"""
    i, d = ((B,), np.int32), ((B,), np.float64)
    return dict(gate=i, quality=i, result=i, T_out=((B, 12), np.float64), nobs_out=i, depth_mean=d, depth_min=d, kf_block=i,
                valid=((B, n_stride), np.uint8), xyz_ref=((B, n_stride, 3), np.float64), key_pts=((B, 5), np.int32),
                occupancy=((B, cells), np.uint8), kf_remove=i)


def params_struct(capi, params):
    p = capi.FrameCloseParams(**{k: v for k, v in dict(chk.DEFAULTS, **params).items()})
    return p
