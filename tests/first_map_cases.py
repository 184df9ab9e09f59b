"""TEST INFRASTRUCTURE.  The cases of the K10 tests (numpy only): what K8 / K9 and the gates leave for n sequences, built by
hand so that every rule of svo_hip_first_map / svo_hip_initialize_seeds (include/svo_hip.h) is exercised on the smallest
shapes at which it can go wrong; the checker's answer per batch (tests/first_map_checker.py, computed once per process);
the comparison rule of the GPU tests.

Corners that are not point_ok carry NaN points, NaN bearings and pixels of -777: nothing of theirs may be read.  Pixels are
f32; poses are random rotations of up to 3 rad, so all four branches of the quaternion conversion occur.

Comparison: `compare_bits` of tests/host_buffers.py -- every output bit for bit (the emulated kernel; the reference's arithmetic
is IEEE f64 with one rounding per operation, and so is the emulation's).  `compare_device` -- the GPU rule: discrete outputs equal, f64 ones
within 1e-14 relative (each value is a chain of under ten IEEE operations: about 45 ulp of headroom), f32 seed fields within
1 ulp; returns the largest differences so that the tests can print them."""
import functools
import types

import numpy as np

import first_map_checker as chk
from homography_cases import rodrigues
from host_buffers import relative_difference, same_bits

INPUTS = ("result", "point_ok", "point_w", "px_ref", "px_cur", "f_ref", "f_cur", "T_ref_w", "T_cur_w")
DISCRETE = ("n_points", "src_index", "key_pts", "occupancy")
CONTINUOUS = ("pos", "px", "f", "depth_mean", "depth_min", "xyz_ref")
SEED_DISCRETE = ("n_seeds", "frame", "level", "type", "batch_id")
SEED_F64 = ("px", "f", "grad")
SEED_F32 = ("a", "b", "mu", "z_range", "sigma2")
F64_BOUND = 1e-14
F32_ULPS = 1
ROUNDED_UP_THRESHOLDS = (20.1, 0.1)


def camera(width, height):
    return types.SimpleNamespace(width=width, height=height, fx=0.9 * width, fy=0.9 * width, cx=width / 2 - 0.5, cy=height / 2 - 0.5,
                                 model=0, d=(0.0,) * 5)


def grid(cam, cell_size):
    """(cell_size, n_cols, n_rows) as FastDetector forms them"""
    return cell_size, -(-cam.width // cell_size), -(-cam.height // cell_size)


def bearing(cam, px):
    px = np.asarray(px, np.float64)
    f = np.stack([(px[:, 0] - cam.cx) / cam.fx, (px[:, 1] - cam.cy) / cam.fy, np.ones(len(px))], axis=1)
    return f / np.linalg.norm(f, axis=1, keepdims=True)


def make_seq(cam, seed, n_pts, n_points, result=chk.SUCCESS, identity=False):
    """n_points point_ok corners spread over n_pts, random pixels inside the image, points in front of the current frame"""
    rng = np.random.default_rng(seed)
    s = types.SimpleNamespace(cam=cam, n_pts=n_pts, result=np.int32(result))
    s.point_ok = np.zeros(n_pts, np.uint8)
    s.point_ok[rng.permutation(n_pts)[:n_points]] = 1
    idx = np.flatnonzero(s.point_ok)
    s.px_ref, s.px_cur = np.full((n_pts, 2), -777.0, np.float32), np.full((n_pts, 2), -777.0, np.float32)
    for px in (s.px_ref, s.px_cur):
        px[idx] = np.stack([rng.uniform(0, cam.width - 1, n_points), rng.uniform(0, cam.height - 1, n_points)], axis=1).astype(np.float32)
    s.f_ref, s.f_cur = np.full((n_pts, 3), np.nan), np.full((n_pts, 3), np.nan)
    s.f_ref[idx], s.f_cur[idx] = bearing(cam, s.px_ref[idx]), bearing(cam, s.px_cur[idx])
    axis = rng.normal(size=3)
    R = np.eye(3) if identity else rodrigues(axis / np.linalg.norm(axis) * rng.uniform(0.0, 3.0))
    t = rng.uniform(-1, 1, 3)
    s.T_cur_w = np.concatenate([R.reshape(9), t])
    aw = rng.normal(size=3)
    s.T_ref_w = np.concatenate([rodrigues(aw / np.linalg.norm(aw) * 0.3).reshape(9), rng.uniform(-1, 1, 3)])
    in_cur = s.f_cur[idx] * rng.uniform(0.5, 4.0, (n_points, 1))
    s.point_w = np.full((n_pts, 3), np.nan)
    s.point_w[idx] = (in_cur - t) @ R                  # R' (x - t)
    return s


def set_pixels(s, view, ranks, pixels, with_bearing=True):
    """the pixels of the given ranks (positions among the point_ok corners) of view 0 / 1, with their bearings"""
    idx = np.flatnonzero(s.point_ok)[np.asarray(ranks)]
    px, f = (s.px_ref, s.f_ref) if view == 0 else (s.px_cur, s.f_cur)
    px[idx] = np.asarray(pixels, np.float32)
    if with_bearing:
        f[idx] = bearing(s.cam, px[idx])


def on_the_centre_lines(cam, seed):
    """features exactly on cu, on cv and on px[0] == cv; features in no quadrant (cv <= px[0] < cu on a wide image) and in
    two (cu <= px[0] < cv on a tall one); the image centre itself twice (a tie for key point 0, products of +0 and -0)"""
    s = make_seq(cam, seed, 70, 40)
    cu, cv = cam.width // 2, cam.height // 2
    lo, hi = min(cu, cv), max(cu, cv)
    between = (lo + hi) / 2.0
    special = [(cu, cv), (cu, cv), (cu, 1.0), (cu, cam.height - 2.0), (1.0, cv), (cam.width - 2.0, cv), (cv, cv), (cv, 2.0), (cv, cam.height - 3.0),
               (between, 3.0), (between, cam.height - 3.0), (cu - 0.5, cv - 0.5), (cu + 0.5, cv - 0.5), (cu - 0.5, cv + 0.5), (cu + 0.5, cv + 0.5)]
    for view in (0, 1):
        set_pixels(s, view, np.arange(3, 3 + len(special)), special)
    return s


def only_between(cam, seed):
    """every feature has lo <= px[0] < hi (lo, hi = cv, cu in either order): on a wide image key points 1..4 are all NULL,
    on a tall one every feature is in two quadrants"""
    s = make_seq(cam, seed, 20, 12)
    cu, cv = cam.width // 2, cam.height // 2
    lo, hi = min(cu, cv), max(cu, cv)
    rng = np.random.default_rng(seed + 1)
    for view in (0, 1):
        set_pixels(s, view, np.arange(12), np.stack([rng.uniform(lo, hi - 0.01, 12), rng.uniform(0, cam.height - 1, 12)], axis=1))
    return s


def duplicated_pixels(cam, seed):
    """the second half of the features repeats the pixels of the first half, in reverse order: a tie for every key point"""
    s = make_seq(cam, seed, 130, 100)
    idx = np.flatnonzero(s.point_ok)
    for px, f in ((s.px_ref, s.f_ref), (s.px_cur, s.f_cur)):
        px[idx[50:]] = px[idx[:50]][::-1]
        f[idx[50:]] = f[idx[:50]][::-1]
    return s


def equal_depths(cam, seed, n_points):
    """identity rotation; five points around the median rank share one depth, and so do the two smallest"""
    s = make_seq(cam, seed, n_points + 7, n_points, identity=True)
    idx = np.flatnonzero(s.point_ok)
    z = s.point_w[idx, 2].copy()
    order = np.argsort(z)
    mid = n_points // 2
    z[order[max(mid - 2, 0):mid + 3]] = z[order[mid]]
    if n_points > 1:
        z[order[1]] = z[order[0]]
    s.point_w[idx, 2] = z
    return s


def bad_pixels(cam, seed, cell_size):
    """point_ok set by hand on corners whose current pixel is NaN, infinite, negative by more than a cell, beyond the grid
    in x, in y, or huge; one pixel inside (-cell_size, 0) (truncates to cell 0, as in the reference) and one on the last
    cell's far edge.  The stored bearings stay those of the original pixels."""
    s = make_seq(cam, seed, 40, 24)
    _, n_cols, n_rows = grid(cam, cell_size)
    bad = [(np.nan, 5.0), (5.0, np.nan), (np.inf, 5.0), (5.0, -np.inf), (-cell_size - 1.0, 5.0), (5.0, -2.0 * cell_size), (n_cols * cell_size, 5.0),
           (5.0, n_rows * cell_size), (1e30, 5.0), (5.0, -1e30), (3e9, 3e9), (-0.5 * cell_size, 5.0), (n_cols * cell_size - 0.25, n_rows * cell_size - 0.25)]
    set_pixels(s, 1, np.arange(2, 2 + len(bad)), bad, with_bearing=False)
    # (the reference frame's pixels only feed its key points; a NaN on rank 0 stays key point 0: nothing is strictly nearer)
    set_pixels(s, 0, [0, 4, 5], [(np.nan, np.nan), (np.nan, 3.0), (-np.inf, 7.0)], with_bearing=False)
    s.n_bad = len(bad)
    return s


def _batch(name, seqs, cell_size):
    cam = seqs[0].cam
    assert len({s.n_pts for s in seqs}) == 1 and all(s.cam is cam for s in seqs)
    return types.SimpleNamespace(name=name, seqs=seqs, cam=cam, n_pts=seqs[0].n_pts, grid=grid(cam, cell_size))


EQUAL_DEPTH_COUNTS = (1, 2, 5, 6, 31, 32)
CAMERAS = {"160x120": (camera(160, 120), 30), "150x118": (camera(150, 118), 30), "47x33": (camera(47, 33), 10), "33x47": (camera(33, 47), 10)}


@functools.lru_cache(maxsize=None)
def batches():
    """name -> batch, with the checker's answer as .expect.  (Built once per process; the tests never write the arrays.)"""
    out = []
    wide, odd, tiny, tall = (CAMERAS[k] for k in ("160x120", "150x118", "47x33", "33x47"))
    # sizes around the strides of the loops (64 lanes, 256 work-items, 1024 corners): n_points 0, 1, n_pts, odd and even
    for k, n_pts in enumerate((1, 63, 64, 65, 255, 256, 257, 1024)):
        cam, cell = (wide, odd, tiny)[k % 3]
        counts = sorted({0, 1, n_pts, n_pts // 2, max(n_pts // 2 - 1, 0), (2 * n_pts) // 3})
        out.append(_batch(f"n{n_pts}", [make_seq(cam, 1000 * n_pts + c, n_pts, c) for c in counts], cell))
    for key, (cam, cell) in CAMERAS.items():
        out.append(_batch(f"centre_lines_{key}", [on_the_centre_lines(cam, 7), on_the_centre_lines(cam, 9)], cell))
        out.append(_batch(f"between_{key}", [only_between(cam, 8)], cell))
        out.append(_batch(f"ties_{key}", [duplicated_pixels(cam, 11)], cell))
    for n in EQUAL_DEPTH_COUNTS:
        out.append(_batch(f"equal_depths_{n}", [equal_depths(odd[0], 20 + n, n)], odd[1]))
    # a sequence without SUCCESS (FAILURE, NO_KEYFRAME, and a value that is no InitResult) between identical SUCCESS ones
    a = make_seq(wide[0], 31, 90, 61)
    fails = [make_seq(wide[0], 32 + r, 90, 50, result=r) for r in (0, 1, 3)]
    out.append(_batch("failed_between", [a, fails[0], a, fails[1], fails[2], a], wide[1]))
    # sixteen sequences: the XCD-contiguous workgroup order is a permutation there (workgroup 1 takes sequence 2)
    out.append(_batch("sixteen", [make_seq(tiny[0], 40 + (i % 3), 70, 20 + 9 * (i % 3)) for i in range(16)], tiny[1]))
    for key, (cam, cell) in CAMERAS.items():
        out.append(_batch(f"bad_pixels_{key}", [bad_pixels(cam, 51, cell)], cell))
    out = {b.name: b for b in out}
    for b in out.values():
        inp = inputs(b)
        b.expect = chk.first_map(b.cam, *[inp[k] for k in INPUTS if k != "T_ref_w"], *b.grid)
    return out


def _names():
    n = [f"n{m}" for m in (1, 63, 64, 65, 255, 256, 257, 1024)]
    for key in ("160x120", "150x118", "47x33", "33x47"):
        n += [f"centre_lines_{key}", f"between_{key}", f"ties_{key}", f"bad_pixels_{key}"]
    return tuple(n + [f"equal_depths_{k}" for k in EQUAL_DEPTH_COUNTS] + ["failed_between", "sixteen"])


NAMES = _names()


def inputs(b):
    """the arrays of a batch as the entry takes them, by name"""
    dt = dict(result=np.int32, point_ok=np.uint8, px_ref=np.float32, px_cur=np.float32)
    return {k: np.ascontiguousarray(np.stack([getattr(s, k) for s in b.seqs]), dtype=dt.get(k, np.float64)) for k in INPUTS}


def out_shapes(n_seq, n_pts, cells):
    """name -> (shape, dtype) of svo_hip_first_map_out, in the struct's order"""
    return dict(n_points=((n_seq,), np.int32), src_index=((n_seq, n_pts), np.int32), pos=((n_seq, n_pts, 3), np.float64),
                px=((n_seq, 2, n_pts, 2), np.float64), f=((n_seq, 2, n_pts, 3), np.float64), key_pts=((n_seq, 2, 5), np.int32),
                depth_mean=((n_seq,), np.float64), depth_min=((n_seq,), np.float64), xyz_ref=((n_seq, n_pts, 3), np.float64),
                occupancy=((n_seq, cells), np.uint8))


def ulp_difference(got, want):
    """the largest distance in f32 representations between two f32 arrays; equal bits count as 0"""
    g, w = np.ascontiguousarray(got, np.float32).ravel(), np.ascontiguousarray(want, np.float32).ravel()
    if same_bits(g, w):
        return 0
    order = lambda a: np.where(a.view(np.int32) < 0, np.int64(-2**31) - a.view(np.int32).astype(np.int64), a.view(np.int32).astype(np.int64))
    bad = np.isnan(g) != np.isnan(w)
    return int(2**40) if bad.any() else int(np.abs(np.where(np.isnan(g), 0, order(g) - order(w))).max())


def compare_device(got, want, discrete, f64, f32=(), what=""):
    """-> (largest relative difference of an f64 output, largest ulp distance of an f32 output), after asserting the rule"""
    for k in discrete:
        assert np.array_equal(np.asarray(got[k]).reshape(np.shape(want[k])), want[k]), (what, k)
    worst = max([relative_difference(got[k], want[k]) for k in f64] + [0.0])
    ulps = max([ulp_difference(got[k], want[k]) for k in f32] + [0])
    assert worst <= F64_BOUND, (what, worst)
    assert ulps <= F32_ULPS, (what, ulps)
    return worst, ulps


# ---- svo_hip_initialize_seeds ------------------------------------------------------------------------------------------------
def make_corners(seed, n_frames, n_cells, fill, cam, threshold=20.0):
    """what svo_hip_fast_detect leaves: fill = the fraction of cells with a corner (0: none, 1: every cell); empty cells hold
    xy = -1, level = -1 and score == float(threshold) -- above the double for 20.1 and 0.1, and still no corner: the level
    says so -- and a few full-looking cells (level 0) score exactly the threshold (not a corner: the test is >)"""
    rng = np.random.default_rng(seed)
    c = types.SimpleNamespace(n_frames=n_frames, n_cells=n_cells, threshold=threshold, cam=cam)
    has = rng.uniform(size=(n_frames, n_cells)) < fill
    c.xy = np.where(has[..., None], np.stack([rng.integers(0, cam.width, (n_frames, n_cells)), rng.integers(0, cam.height, (n_frames, n_cells))],
                                             axis=-1), -1).astype(np.int32)
    c.level = np.where(has, rng.integers(0, 3, (n_frames, n_cells)), -1).astype(np.int32)
    c.score = np.where(has, rng.uniform(threshold, 200.0, (n_frames, n_cells)), threshold).astype(np.float32)
    if fill and n_cells > 4:
        at = np.float32(threshold)                      # the largest float that is not above the threshold: the threshold itself at 20.0
        c.score[:, 3] = at if float(at) <= threshold else np.nextafter(at, np.float32(0))
        c.xy[:, 3] = (5, 6)
        c.level[:, 3] = 0
    c.frame_index = (np.arange(n_frames) * 3 + 2).astype(np.int32)
    c.depth_mean = rng.uniform(0.5, 5.0, n_frames)
    c.depth_min = rng.uniform(0.1, 0.5, n_frames)
    return c


@functools.lru_cache(maxsize=None)
def seed_cases():
    """name -> (corners, seed_stride, batch_id), with the checker's answer as corners.expect"""
    cam = CAMERAS["160x120"][0]
    out = {}
    for n_cells in (1, 255, 256, 257, 1040):
        out[f"cells{n_cells}"] = (make_corners(n_cells, 3, n_cells, 0.6, cam), n_cells, 1)
    out["no_corner"] = (make_corners(5, 2, 257, 0.0, cam), 257, 2)
    out["every_corner"] = (make_corners(6, 2, 257, 1.0, cam), 257, 3)
    out["wide_stride"] = (make_corners(7, 2, 70, 0.5, cam), 100, 4)
    out["one_cell_full"] = (make_corners(8, 1, 1, 1.0, cam), 1, 1)
    zero = make_corners(9, 8, 24, 0.7, cam)
    zero.depth_mean[1], zero.depth_min[1] = 0.0, 0.0          # a failed sequence's scene depth: mu = z_range = sigma2 = inf
    out["eight_frames_zero_depth"] = (zero, 24, 5)
    # thresholds whose float lies above the double (20.100000381 > 20.1): an empty cell's score passes "score > threshold"
    # and its level, -1, must keep it from becoming a record
    for threshold in ROUNDED_UP_THRESHOLDS:
        assert float(np.float32(threshold)) > threshold
        out[f"threshold_{threshold}"] = (make_corners(10, 3, 257, 0.5, cam, threshold=threshold), 257, 6)
    for c, stride, batch_id in out.values():
        c.expect = chk.initialize_seeds(c.cam, c.xy, c.level, c.score, c.threshold, c.frame_index, c.depth_mean, c.depth_min, batch_id, stride)
    return out


def check_seed_rule(c, got):
    """K7's rule, read off the inputs and not off the checker (which states the same rule as the kernel): one record per cell
    with level >= 0 whose score beats the threshold, none for an empty cell (level -1, pixel -1), whatever its score"""
    corner = (c.level >= 0) & (c.score.astype(np.float64) > c.threshold)
    n = got["n_seeds"]
    assert np.array_equal(n, corner.sum(axis=1)), (n, corner.sum(axis=1))
    for f in range(c.n_frames):
        assert (got["level"][f, :n[f]] >= 0).all() and (got["px"][f, :n[f]] >= 0).all(), f
        assert np.array_equal(got["px"][f, :n[f]], c.xy[f][corner[f]].astype(np.float64)), f
    return n


SEED_NAMES = ("cells1", "cells255", "cells256", "cells257", "cells1040", "no_corner", "every_corner", "wide_stride", "one_cell_full",
              "eight_frames_zero_depth") + tuple(f"threshold_{t}" for t in ROUNDED_UP_THRESHOLDS)
