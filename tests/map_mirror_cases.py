"""TEST INFRASTRUCTURE, not a test.  The named cases, the builder conditions and the ONE comparison rule of the map-mirror edge
tests -- tests/test_map_mirror_rules.py (the rule against mutants of the walk), tests/test_map_mirror_edges_emulated.py,
tests/test_map_mirror_edges_gpu.py and tests/test_map_mirror_sanitized.py -- for svo_hip_reproject_map
(rpg_svo_amd/csrc/map_mirror.hip).  The references are tests/map_walk_reference.py (the independent walk, mpmath) and the
oracle's orc_reproject_map.  numpy, mpmath, ctypes, rpg_svo_amd.se3 / synth and helpers: nothing here touches a GPU or loads a
library under test.

A case (case(name, kind)) is a camera and a list of Steps: a plain-array map as helpers.random_map returns it plus the call's
parameters; a Step with `touched` is a second call on the same mirror whose patch carries those entries.  Shapes are the
smallest that reach the path; every launch is one workgroup.

  records_8_and_9   15-frame table, 200 points with exactly 8 observation records and 200 with exactly 9: the eight records a
                    thread fetches at once, and the first one of the loop behind them
  many_views        14 keyframes, 300 points seen from 9..14 of them, records shuffled, 3 and 10 overlapping keyframes: the
                    first meeting and the chosen observation at record index >= 8, records in keyframes without overlap (they
                    count for the close view, never for the first meeting)
  crowded_cell      more than 600 entries of the three types interleaved in one cell (the O(n^2) rank of one thread), its eight neighbours
                    empty, a cell with a single entry
  behind_camera     80 points with negative depth in the current frame; reprojectPoint has no depth test, their mirrored
                    projections are binned
  key_limits        64-frame table, ranks 0..15, fts_ positions 0 and 4095 in one keyframe, candidate orders 0 and 64999, the
                    current frame a middle row
  small_cells       640x480, cell_size 13: 1850 cells, a thread's second cell in the ordering step
  cell_limit        640x320, cell_size 10: exactly 2048 cells, the last visiting rank populated
  exact_edges       dyadic pinhole, identity pose, depths 1, 2, 4: px EXACTLY on the isInFrame limits (8, w - 8, h - 8) and on a
                    cell boundary (30), and 2^-20 px on either side
  close_view_ties   two keyframes with bit-identical poses (equal cosines: the first record wins), a point whose observers all
                    give cos <= 0 (first record, no view), a binned candidate without observations (a visit, never a trial), and
                    a point whose best cosine is 0.5 exactly -- in real arithmetic (4 (a.b)^2 = |a|^2 |b|^2 in integers) and in
                    the doubles of `v / sqrt(v.v)` and a left-to-right dot product, which the builder evaluates
  in_frame_limit    4096 and 4097 points inside the frame out of 4096 (four entries per thread, all of them binned), 4097 (eight
                    per thread) and 8192 entries: status 1 beyond 4096, nothing written to the visit and trial arrays
  cuts              one map through max_cells_with_trials 0, 1, N, N + 1 and first_cell 0, middle, the last cell with a trial,
                    n_cells; a cut and its continuation from end_cell
  capacities        max_visits in {V, V - 1}, max_trials in {M, M - 1}: one slot short is status 1 with V = M = 0
  patch_moves_first_meeting   a patch that rewrites observation records (points change the keyframe they are first met
                    through: kf_count moves), kills entries and promotes others

Builder conditions, asserted where the cases are built (a case that misses one is a mistake of this file):
  * outside exact_edges no projected px lies within camera_cases.CELL_MARGIN (1e-7 px) of a border or a cell edge that decides
    its cell; in exact_edges every px is exactly the intended double (asserted in mpmath) or 2^-20 px from it;
  * outside close_view_ties no |cos - 0.5| of a visited point and no gap between its best cosine and the next (another frame's,
    or 0) is below COS_MARGIN = 1e-9 -- a double evaluation of the cosine is good to a few 1e-16;
  * per case what its row above promises (counts, indices >= 8, ranks used, ...).
No case is exempt from the integer comparison.

Outside the header's contract and UNASSERTED: d_kf_rank values >= 16, fts_ positions >= 4096, candidate orders >= 65000
(rpg_svo_amd/host/dropin/map_mirror.h refuses them before they reach the mirror), and a cosine within 1e-9 of 0.5 other than the
one exact case above.

The rule (check_step): every integer output -- header, point_cell, kf_count, visit_*, trial_obs_begin / end, trial_cell,
trial_cur -- identical to the independent walk AND to the oracle, nothing masked; trial_pos bit for bit; point_px and trial_px
within `px_tol_oracle` of the oracle (1e-9 px on the device, 1e-12 in emulation: the bounds of tests/test_map_mirror_gpu.py and
tests/test_map_mirror_emulated.py) and within camera_cases.PIXEL_ATOL + PIXEL_RTOL |px| of the mpmath walk (check_pixels' bound
for svo_hip_reproject_points: the same arithmetic).  Outputs start poisoned (Outputs: ints 0x55555555, doubles NaN, guard words
around every array): what the entry defines it writes, d_point_px stays untouched where d_point_cell == -2, nothing is written
beyond V visits and M trials, and a status-1 call writes no visit and no trial at all."""
import ctypes as C
import functools
import struct
from dataclasses import dataclass, field

import numpy as np

import camera_cases as cc
import map_walk_reference as W
from camera_reference import mpf
from helpers import camera_models, fuzz_rng, oracle_reproject_map, random_map
from rpg_svo_amd import capi, se3, synth

COS_MARGIN = 1e-9
MAX_IN_FRAME = capi.REPROJ_MAX_IN_FRAME
OK, EINVAL, ERANGE = 0, -1, -2
R0 = np.diag([1.0, -1.0, -1.0])      # a camera above the plane z = 0, looking down
CUR_CENTRE = np.array([0.1, -0.2, 2.0])

CASE_NAMES = ("records_8_and_9", "many_views", "crowded_cell", "behind_camera", "key_limits", "small_cells", "cell_limit", "exact_edges",
              "close_view_ties", "in_frame_limit", "cuts", "capacities", "patch_moves_first_meeting")
ALL_CAMERAS = ("many_views", "behind_camera")     # these run on radtan and atan too
CASES = [(n, "pinhole") for n in CASE_NAMES] + [(n, k) for n in ALL_CAMERAS for k in ("radtan", "atan")]
CASE_IDS = [f"{n}-{k}" for n, k in CASES]
SANITIZED = ("crowded_cell", "in_frame_limit", "cell_limit", "key_limits")


@dataclass
class Step:
    mp: dict
    first_cell: int = 0
    max_cells: int = 1 << 30
    max_visits: int = MAX_IN_FRAME
    max_trials: int = MAX_IN_FRAME
    touched: np.ndarray = None        # None: a new mirror, the whole map uploaded; else the entries the patch carries
    touched_obs: np.ndarray = None
    label: str = ""


@dataclass
class Case:
    name: str
    kind: str
    cam: object
    steps: list
    exact_px: bool = False
    tied_cos: bool = False
    extra: object = None              # extra(outs): what the case asserts across its steps
    facts: dict = field(default_factory=dict)


# ---- building maps -----------------------------------------------------------------------------------------------------------
def _pose(R, centre):
    return se3.join(R, -R @ np.asarray(centre, np.float64))


def _poses(rng, n_frames, cur, spread=3.0):
    """keyframe centres up to `spread` m from the current one at ~2 m height, looking down, tilted by a few degrees"""
    T = np.zeros((n_frames, 12))
    for i in range(n_frames):
        R = se3.split(se3.exp(np.concatenate([np.zeros(3), rng.normal(0, 0.05, 3)])))[0] @ R0
        ctr = CUR_CENTRE if i == cur else np.array([rng.uniform(-spread, spread), rng.uniform(-spread, spread), rng.uniform(1.6, 2.4)])
        T[i] = _pose(R, ctr)
    return T


def _centres(T):
    return se3.inv(T)[:, 9:]


def _ranks(T, cur, n_overlap):
    """the n_overlap keyframes closest to the current frame, closest = 0"""
    c = _centres(T)
    kfs = np.array([i for i in range(len(T)) if i != cur])
    rank = np.full(len(T), -1, np.int32)
    for r, j in enumerate(np.argsort(np.linalg.norm(c[kfs] - c[cur], axis=1), kind="stable")[:n_overlap]):
        rank[kfs[j]] = r
    return rank


def _plane(cam, rng, n, frac=1.3):
    """points on and around the plane, over `frac` times the field of view"""
    span = frac * max(cam.width / cam.fx, cam.height / cam.fy)
    return np.stack([rng.uniform(-span, span, n) + CUR_CENTRE[0], rng.uniform(-span, span, n) + CUR_CENTRE[1], rng.normal(0, 0.05, n)], -1)


def _at_pixel(cam, T_row, u, v, depth):
    """world points at `depth` in the frame whose projections are (about) the pixels (u, v); depth < 0: mirrored into them"""
    x, y = synth.cam_undistort(cam, np.asarray(u, np.float64), np.asarray(v, np.float64))
    q = np.stack([x * depth, y * depth, np.broadcast_to(np.asarray(depth, np.float64), np.shape(x))], -1)
    R, t = se3.split(T_row)
    return (q - t) @ R


class _Map:
    """collects points (position, type, records) and turns them into the plain-array map"""

    def __init__(self, cam, T, cur, kf_rank, rng, cell_size=30):
        self.cam, self.T, self.cur, self.kf_rank, self.rng, self.cell_size = cam, T, cur, np.asarray(kf_rank, np.int32), rng, cell_size
        self.pts, self._free = [], {}
        self.kfs = [i for i in range(len(T)) if i != cur]

    def slot(self, f):
        """a position in keyframe f's fts_ nobody has yet (1..4094: the limits are given out by hand)"""
        if f not in self._free:
            self._free[f] = list(self.rng.permutation(np.arange(1, 4095)))
        return int(self._free[f].pop())

    def point(self, pos, type_, frames, positions=None):
        recs = [(int(f), self.slot(f) if positions is None or positions[i] is None else int(positions[i])) for i, f in enumerate(frames)]
        self.pts.append((np.asarray(pos, np.float64), int(type_), 0, recs))
        return len(self.pts) - 1

    def candidate(self, pos, order, frame=None):
        self.pts.append((np.asarray(pos, np.float64), 1, int(order), [] if frame is None else [(int(frame), -1)]))
        return len(self.pts) - 1

    def build(self, cell_order=None):
        cam, rng = self.cam, self.rng
        P = len(self.pts)
        obs_begin, obs_count, obs_frame, obs_order = np.zeros(P, np.int32), np.zeros(P, np.int32), [], []
        for p, (_, _, _, recs) in enumerate(self.pts):
            obs_begin[p], obs_count[p] = len(obs_frame), len(recs)
            obs_frame += [f for f, _ in recs]
            obs_order += [o for _, o in recs]
        O = len(obs_frame)
        n_cols, n_rows = -(-cam.width // self.cell_size), -(-cam.height // self.cell_size)
        if cell_order is None:
            cell_order = rng.permutation(n_cols * n_rows)
        cell_rank = np.empty(n_cols * n_rows, np.int32)
        cell_rank[cell_order] = np.arange(n_cols * n_rows, dtype=np.int32)
        return dict(T=np.ascontiguousarray(self.T), cur=self.cur, kf_rank=self.kf_rank, pos=np.array([x[0] for x in self.pts]).reshape(P, 3),
                    type=np.array([x[1] for x in self.pts], np.int32), order=np.array([x[2] for x in self.pts], np.int32),
                    obs_begin=obs_begin, obs_count=obs_count, obs_frame=np.array(obs_frame, np.int32), obs_order=np.array(obs_order, np.int32),
                    obs_level=rng.integers(0, 3, O).astype(np.int32), obs_type=(rng.uniform(size=O) < 0.2).astype(np.uint8),
                    obs_px=rng.uniform(20, 400, (O, 2)), obs_f=rng.normal(size=(O, 3)), obs_grad=rng.normal(size=(O, 2)),
                    cell_size=self.cell_size, n_cols=n_cols, n_rows=n_rows, cell_order=np.asarray(cell_order), cell_rank=cell_rank)


def _copy(mp):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in mp.items() if not k.startswith("_")}


def _walk(step, cam):
    return W.REF_WALK.walk(step.mp, cam, step.first_cell, step.max_cells)


def _record_index(mp, p, o):
    return int(o) - int(mp["obs_begin"][p])


def _first_meetings(mp):
    """per point the record through which the keyframe loop meets it first (-1: never), by the definition of svo_hip.h:
    smallest (rank, position) over its records in overlapping keyframes"""
    out = np.full(mp["pos"].shape[0], -1, np.int64)
    for p in range(mp["pos"].shape[0]):
        if mp["type"][p] < 2:
            continue
        best = None
        for o in range(mp["obs_begin"][p], mp["obs_begin"][p] + mp["obs_count"][p]):
            r = mp["kf_rank"][mp["obs_frame"][o]]
            if r >= 0 and mp["obs_order"][o] >= 0 and (best is None or (r, mp["obs_order"][o]) < best[0]):
                best = ((r, mp["obs_order"][o]), o)
        if best:
            out[p] = best[1]
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def _records_8_and_9(cam, rng):
    T = _poses(rng, 15, 14)
    m = _Map(cam, T, 14, _ranks(T, 14, 10), rng)
    pos = _plane(cam, rng, 400)
    for i in range(400):
        m.point(pos[i], rng.choice([2, 3]), rng.permutation(14)[:8 + i % 2])
    for i, x in enumerate(_plane(cam, rng, 60)):
        m.candidate(x, i, rng.integers(14))
    mp = m.build()
    assert (mp["obs_count"][:400] == 8).sum() == 200 and (mp["obs_count"][:400] == 9).sum() == 200
    w = W.REF_WALK.walk(mp, cam)
    last = [p for p, o in zip(w["visit_point"][w["visit_trial"] >= 0], w["trial_obs"]) if p < 400 and _record_index(mp, p, o) == mp["obs_count"][p] - 1]
    assert len(last) >= 10, len(last)      # the last record (index 7 or 8) is the chosen one for some
    return [Step(mp)], {}


def _many_views(cam, rng, kind):
    steps, facts = [], {}
    for n_overlap in (3, 10):
        T = _poses(rng, 15, 14)
        rank = _ranks(T, 14, n_overlap)
        m = _Map(cam, T, 14, rank, rng)
        pos = _plane(cam, rng, 300, frac=1.0)
        c = _centres(T)
        over, rest = [f for f in range(14) if rank[f] >= 0], [f for f in range(14) if rank[f] < 0]
        for i in range(300):
            k = int(rng.integers(9, 15))
            frames = list(rng.permutation(14)[:k])
            group = i % 4
            if group == 1 and any(rank[f] >= 0 for f in frames):      # the first meeting at the last index
                first = min((f for f in frames if rank[f] >= 0), key=lambda f: rank[f])
                frames.remove(first); frames.append(first)
            elif group == 2:                                           # the best view at the last index
                d = c[frames] - pos[i]
                cosv = (d @ (c[14] - pos[i])) / np.linalg.norm(d, axis=1)
                best = frames[int(np.argmax(cosv))]
                frames.remove(best); frames.append(best)
            elif group == 3 and n_overlap == 3:                        # one record in an overlapping keyframe, the last one
                frames = list(rng.permutation(rest)[:int(rng.integers(8, len(rest) + 1))]) + [int(rng.choice(over))]
            m.point(pos[i], rng.choice([2, 3]), frames)
        mp = m.build()
        w = W.REF_WALK.walk(mp, cam)
        meet = _first_meetings(mp)
        late_meet = sum(1 for p in range(300) if w["point_cell"][p] >= -1 and _record_index(mp, p, meet[p]) >= 8)
        late_view = sum(1 for p, o in zip(w["visit_point"][w["visit_trial"] >= 0], w["trial_obs"]) if _record_index(mp, p, o) >= 8)
        assert late_meet >= 40 and late_view >= 40, (n_overlap, late_meet, late_view)
        facts[f"late_meet_{n_overlap}"], facts[f"late_view_{n_overlap}"] = late_meet, late_view
        if n_overlap == 3:
            only = 0
            for p in range(300):
                idx = [o - mp["obs_begin"][p] for o in range(mp["obs_begin"][p], mp["obs_begin"][p] + mp["obs_count"][p])
                       if rank[mp["obs_frame"][o]] >= 0]
                only += len(idx) == 1 and idx[0] >= 8 and w["point_cell"][p] >= -1
            assert only >= 5, only     # a kernel that dropped that record would report -2
            facts["only_record_late"] = int(only)
            far = sum(1 for p, o in zip(w["visit_point"][w["visit_trial"] >= 0], w["trial_obs"]) if rank[mp["obs_frame"][o]] < 0)
            assert far >= 40, far      # the chosen observation is in a keyframe without overlap
        steps.append(Step(mp, label=f"n_overlap {n_overlap}"))
    return steps, facts


def _crowded_cell(cam, rng):
    T = _poses(rng, 9, 8)
    m = _Map(cam, T, 8, _ranks(T, 8, 6), rng)
    col, row, n = 10, 8, 720
    u, v = rng.uniform(30 * col + 1, 30 * col + 29, n), rng.uniform(30 * row + 1, 30 * row + 29, n)
    pos = _at_pixel(cam, T[8], u, v, rng.uniform(1.9, 2.1, n))
    orders = rng.permutation(n)
    for i in range(n):     # good, unknown, candidate, good, ... : the types interleaved in entry order
        if i % 3 == 2:
            m.candidate(pos[i], orders[i], rng.integers(8))
        else:
            m.point(pos[i], 3 - i % 3, rng.permutation(8)[:int(rng.integers(1, 4))])
    m.point(_at_pixel(cam, T[8], 75.0, 400.0, 2.0), 2, [int(np.argmin(np.where(m.kf_rank[:8] >= 0, m.kf_rank[:8], 99)))])
    mp = m.build()
    w = W.REF_WALK.walk(mp, cam)
    crowded, single = row * mp["n_cols"] + col, (400 // 30) * mp["n_cols"] + 75 // 30
    counts = np.bincount(w["point_cell"][w["point_cell"] >= 0], minlength=mp["n_cols"] * mp["n_rows"])
    assert counts[crowded] >= 600 and counts[single] == 1 and counts.sum() == counts[crowded] + 1, (counts[crowded], counts[single], counts.sum())
    in_cell = mp["type"][w["point_cell"] == crowded]
    assert all((in_cell == t).sum() >= 100 for t in (1, 2, 3))
    return [Step(mp)], {"crowded": int(counts[crowded])}


def _behind_camera(cam, rng):
    T = _poses(rng, 11, 10)
    m = _Map(cam, T, 10, _ranks(T, 10, 8), rng)
    for x in _plane(cam, rng, 250):
        m.point(x, rng.choice([2, 3]), rng.permutation(10)[:int(rng.integers(1, 5))])
    behind = []
    u, v = rng.uniform(40, cam.width - 40, 50), rng.uniform(40, cam.height - 40, 50)
    back = list(_at_pixel(cam, T[10], u, v, -rng.uniform(0.5, 3.0, 50)))                 # mirrored into the frame
    R, t = se3.split(T[10])                                                                # and anywhere behind it
    back += list((np.stack([-2.0 * rng.uniform(-1.5, 1.5, 30), -2.0 * rng.uniform(-1.2, 1.2, 30), np.full(30, -2.0)], -1) - t) @ R)
    for i, x in enumerate(back):
        if i % 4 == 3:
            behind.append(m.candidate(x, i, rng.integers(10)))
        else:
            behind.append(m.point(x, rng.choice([2, 3]), rng.permutation(10)[:int(rng.integers(1, 5))]))
    for i, x in enumerate(_plane(cam, rng, 60)):
        m.candidate(x, 100 + i, rng.integers(10))
    mp = m.build()
    w = W.REF_WALK.walk(mp, cam)
    geo = W.geometry(mp, cam)
    negative = [p for p in behind if w["point_cell"][p] >= -1 and geo.project(p)[2] < 0]
    binned = [p for p in negative if w["point_cell"][p] >= 0]
    assert len(negative) >= 60 and len(binned) >= 20, (len(negative), len(binned))
    return [Step(mp)], {"behind": len(negative), "behind_binned": len(binned)}


def _key_limits(cam, rng):
    cur = 31
    T = _poses(rng, 64, cur)
    rank = _ranks(T, cur, 16)
    over = [int(np.flatnonzero(rank == r)[0]) for r in range(16)]
    assert min(over) < cur < max(over)                         # keyframe rows on both sides of the current frame
    m = _Map(cam, T, cur, rank, rng)
    pos = _plane(cam, rng, 520, frac=1.0)
    for i in range(500):
        m.point(pos[i], rng.choice([2, 3]), rng.permutation(m.kfs)[:int(rng.integers(1, 7))])
    inside = _at_pixel(cam, T[cur], np.array([100.5, 200.5, 300.5, 400.5, 500.5, 150.5]), np.array([100.5, 150.5, 200.5, 250.5, 300.5, 350.5]), 2.0)
    limits = [m.point(inside[0], 3, [over[15]], [0]), m.point(inside[1], 2, [over[15]], [4095]),      # both limits in one keyframe
              m.point(inside[2], 2, [over[0]], [4095]), m.point(inside[3], 3, [over[0]], [0]),
              m.point(inside[4], 2, [over[15], over[0]], [0, 4095])]                                    # rank 0 at 4095 beats rank 15 at 0
    for i in range(14):
        m.candidate(pos[500 + i], 1000 + 4000 * i, rng.integers(63))
    cands = [m.candidate(inside[5], 64999, m.kfs[0]), m.candidate(inside[5] + [0.3, 0.2, 0.0], 0, m.kfs[5])]
    mp = m.build()
    assert mp["obs_order"].max() == 4095 and mp["obs_order"][mp["obs_order"] >= 0].min() == 0 and mp["order"].max() == 64999
    w = W.REF_WALK.walk(mp, cam)
    assert all(w["point_cell"][p] >= 0 for p in limits + cands)
    assert w["kf_count"][over[0]] > 0 and w["kf_count"][over[15]] >= 2 and w["kf_count"][cur] == 0
    return [Step(mp)], {}


def _small_cells(cam, rng):
    mp = _copy(random_map(cam, n_kfs=10, n_points=900, n_candidates=500, seed=int(rng.integers(1 << 30)), cell_size=13))
    assert (mp["n_cols"], mp["n_rows"]) == (50, 37)
    w = W.REF_WALK.walk(mp, cam)
    assert (w["visit_cell"] >= 1024).sum() > 100 and (w["visit_cell"] < 1024).sum() > 100     # both cells of a thread
    return [Step(mp)], {}


def _cell_limit(cam, rng):
    cam = synth.Camera(640, 320, 400.0, 400.0, 320.0, 160.0)
    T = _poses(rng, 9, 8)
    m = _Map(cam, T, 8, _ranks(T, 8, 6), rng, cell_size=10)
    for x in _plane(cam, rng, 700):
        m.point(x, rng.choice([2, 3]), rng.permutation(8)[:int(rng.integers(1, 5))])
    for i, x in enumerate(_plane(cam, rng, 300)):
        m.candidate(x, i, rng.integers(8))
    mp = m.build()
    assert mp["n_cols"] * mp["n_rows"] == capi.REPROJ_MAX_CELLS
    # the first and the last cell of the visiting order are populated ones (the cells under the 8 px border never are)
    cells = W.REF_WALK.walk(mp, cam)["point_cell"]
    a, b = int(cells[cells >= 0][0]), int(cells[cells >= 0][-1])
    order = [k for k in mp["cell_order"] if k not in (a, b)]
    mp = _copy(mp)
    mp["cell_order"] = np.array([a] + order + [b])
    mp["cell_rank"][mp["cell_order"]] = np.arange(len(mp["cell_order"]), dtype=np.int32)
    w = W.REF_WALK.walk(mp, cam)
    assert a != b and w["visit_cell"][0] == 0 and w["visit_cell"][-1] == capi.REPROJ_MAX_CELLS - 1
    return cam, [Step(mp)], {}


EPS = 2.0 ** -20


def _exact_edges(cam, rng):
    cam = synth.Camera(640, 480, 512.0, 512.0, 320.0, 240.0)
    w_, h_ = cam.width, cam.height
    T = np.stack([_pose(np.eye(3), c) for c in ([0.25, 0.0, 0.0], [-0.25, 0.125, 0.0], [0.0, -0.25, -0.125], [0.0, 0.0, 0.0])])
    m = _Map(cam, T, 3, np.array([1, 0, 2, -1], np.int32), rng)
    want = {}
    us = [8 - EPS, 8.0, 8 + EPS, w_ - 8 - EPS, float(w_ - 8), w_ - 8 + EPS, 30 - EPS, 30.0, 30 + EPS, 300 - EPS, 300.0]
    vs = [8 - EPS, 8.0, 8 + EPS, h_ - 8 - EPS, float(h_ - 8), h_ - 8 + EPS, 30 - EPS, 30.0, 30 + EPS, 240 - EPS, 240.0]
    k = 0
    for axis, values in ((0, us), (1, vs)):
        for val in values:
            for z in (1.0, 2.0, 4.0):
                u, v = (val, 100.25 + 32 * (k % 7)) if axis == 0 else (100.25 + 64 * (k % 7), val)
                pos = np.array([(u - 320.0) / 512.0 * z, (v - 240.0) / 512.0 * z, z])
                if k % 3 == 2:
                    p = m.candidate(pos, k, k % 3)
                else:
                    p = m.point(pos, 2 + k % 2, [k % 3])
                want[p] = (u, v)
                k += 1
    mp = m.build()
    geo = W.geometry(mp, cam)
    for p, (u, v) in want.items():   # the intended pixel is the exact one
        cell, (ur, vr), depth, _ = geo.project(p)
        assert ur == mpf(u) and vr == mpf(v) and depth > 0, (p, u, v)
        inside = 8 <= int(u) < w_ - 8 and 8 <= int(v) < h_ - 8
        assert cell == ((int(v / 30) * mp["n_cols"] + int(u / 30)) if inside else -1), (p, u, v, cell)
    return cam, [Step(mp)], {}


# current centre - point, observer's centre - point: in eighths (-6, -4, 10) and (-10, 6, 4), a.b = 76, |a|^2 = |b|^2 = 152, so
# 4 (a.b)^2 = |a|^2 |b|^2 and the cosine is 1/2
HALF_A, HALF_B = np.array([-0.75, -0.5, 1.25]), np.array([-1.25, 0.75, 0.5])


def _double_cosine(a, b):
    """the reference's arithmetic in doubles: v / sqrt(v.v), then a left-to-right dot product"""
    a, b = a / np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), b / np.sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2])
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _close_view_ties(cam, rng):
    # every pose is R0 exactly with a dyadic centre: Frame::pos() = -R^T t is exact in doubles, so equal poses give equal cosines
    # on every backend and the 0.5 below is the same double everywhere
    cur_c = np.array([0.25, -0.25, 2.0])
    half_p = cur_c - HALF_A
    centres = [[1.0, 0.5, 2.0], [1.0, 0.5, 2.0], [-1.5, 0.75, 1.75], [0.5, -1.0, 2.25], [0.0, 0.0, -2.5], list(half_p + HALF_B), list(cur_c)]
    T = np.stack([_pose(R0, c) for c in centres])
    TWIN_A, TWIN_B, BELOW, HALF_KF, cur = 0, 1, 4, 5, 6
    m = _Map(cam, T, cur, np.array([1, 2, 0, 3, 4, 5, -1], np.int32), rng)
    pos = _plane(cam, rng, 200, frac=0.9) + (cur_c - CUR_CENTRE) * [1, 1, 0]
    twins = []
    for i in range(120):       # the twins in both record orders, alone and among others
        frames = [[TWIN_A, TWIN_B], [TWIN_B, TWIN_A], [2, TWIN_B, TWIN_A], [TWIN_A, 3, TWIN_B]][i % 4]
        twins.append(m.point(pos[i], 2 + i % 2, frames))
    below = [m.point(pos[120 + i], 2 + i % 2, [BELOW] if i % 2 else [BELOW, BELOW]) for i in range(20)]
    bare = [m.candidate(pos[140 + i], 50 + i) for i in range(10)]          # candidates without an observation
    for i in range(40):
        m.candidate(pos[150 + i], i, rng.integers(4))
    half = m.point(half_p, 3, [HALF_KF])
    mp = m.build()
    w = W.REF_WALK.walk(mp, cam)
    geo = W.geometry(mp, cam)
    trial_of = dict(zip(w["visit_point"].tolist(), w["visit_trial"].tolist()))
    n_tied = 0
    for p in twins:            # equal cosines: where a twin is the best view, the first of the two records is chosen
        cos = geo.cosines(p)
        fr = [int(mp["obs_frame"][mp["obs_begin"][p] + j]) for j in range(len(cos))]
        ia, ib = fr.index(TWIN_A), fr.index(TWIN_B)
        assert cos[ia] == cos[ib]
        if p in trial_of and trial_of[p] >= 0 and cos[ia] == max(cos):
            assert w["trial_obs"][trial_of[p]] == mp["obs_begin"][p] + min(ia, ib)
            n_tied += 1
    assert n_tied >= 30, n_tied
    n_below = sum(1 for p in below if p in trial_of and trial_of[p] == -1 and max(geo.cosines(p)) < -0.1)
    assert n_below >= 5, n_below                                           # observers with cos <= 0 only: a visit, no view
    assert sum(1 for p in bare if p in trial_of) >= 3 and all(trial_of[p] == -1 for p in bare if p in trial_of)
    # the point at cos == 0.5 exactly: in real arithmetic, in mpmath and in doubles
    a8, b8 = (HALF_A * 8).astype(int), (HALF_B * 8).astype(int)
    assert 4 * int(a8 @ b8) ** 2 == int(a8 @ a8) * int(b8 @ b8) and a8 @ b8 > 0
    assert np.array_equal(cur_c - half_p, HALF_A) and np.array_equal(np.array(centres[HALF_KF]) - half_p, HALF_B)
    assert abs(geo.cosines(half)[0] - W.HALF) < W.EQUAL and _double_cosine(HALF_A, HALF_B) == 0.5
    assert trial_of[half] >= 0                                             # `min_cos_angle < 0.5` is false: a trial
    return [Step(mp)], {"tied": n_tied, "below": n_below}


def _all_projected_map(cam, rng, P):
    """P live entries, each of them projected: every keyframe overlaps"""
    n_kfs = 10
    T = _poses(rng, n_kfs + 1, n_kfs)
    m = _Map(cam, T, n_kfs, _ranks(T, n_kfs, n_kfs), rng)
    n_cand = P // 4
    pos = _plane(cam, rng, P, frac=1.05)
    for i in range(P - n_cand):
        m.point(pos[i], 2 + i % 2, rng.permutation(n_kfs)[:int(rng.integers(1, 4))])
    orders = rng.permutation(n_cand)
    for i in range(n_cand):
        m.candidate(pos[P - n_cand + i], orders[i], rng.integers(n_kfs))
    return m.build()


def _with_in_frame(mp, cam, rng, E):
    """the map with exactly E entries inside the frame: outside points are moved onto inside ones (or inside ones far out)"""
    cell = W.REF_WALK.walk(mp, cam, 0, 0)["point_cell"]
    inside, outside = np.flatnonzero(cell >= 0), np.flatnonzero(cell == -1)
    new, onto = _copy(mp), []
    if len(inside) < E:
        move = rng.permutation(outside)[:E - len(inside)]
        onto = rng.choice(inside, len(move))
        new["pos"][move] = mp["pos"][onto]
    else:
        move = rng.permutation(inside)[:len(inside) - E]
        new["pos"][move] += [6.0, 0.0, 0.0]
    # (what mpmath computed for the entries that stay is not computed again)
    W.geometry(new, cam).inherit(W.geometry(mp, cam), np.setdiff1d(np.arange(len(cell)), move), zip(move.tolist(), np.asarray(onto).tolist()))
    assert W.REF_WALK.walk(new, cam, 0, 0)["header"][1] == E
    return new


def _in_frame_limit(cam, rng):
    steps, base = [], {}
    for P, E in ((4096, 4096), (4097, 4096), (4097, 4097), (8192, 4096), (8192, 4097)):
        if P not in base:
            base[P] = _all_projected_map(cam, rng, P)
        mp = _with_in_frame(base[P], cam, rng, E)
        assert mp["pos"].shape[0] == P
        steps.append(Step(mp, label=f"{P} entries, {E} in the frame"))
    return steps, {}


def _cuts(cam, rng):
    mp = _copy(random_map(cam, n_kfs=10, n_points=500, n_candidates=300, seed=int(rng.integers(1 << 30))))
    n_cells = mp["n_cols"] * mp["n_rows"]
    full = W.REF_WALK.walk(mp, cam)
    trial_cells = sorted(set(full["trial_cell"].tolist()))
    N, last = len(trial_cells), trial_cells[-1]
    assert N > 50 and last + 1 < n_cells                    # at exactly N the walk ends at last + 1, not at n_cells
    steps = [Step(mp, 0, k, label=f"max_cells_with_trials {k}") for k in (0, 1, N, N + 1)]
    steps += [Step(mp, f, label=f"first_cell {f}") for f in (0, n_cells // 2, last, n_cells)]
    cut = Step(mp, 0, N // 2, label="cut")
    end = int(W.REF_WALK.walk(mp, cam, 0, N // 2)["header"][4])
    steps += [cut, Step(mp, end, label="continuation")]
    assert W.REF_WALK.walk(mp, cam, 0, N)["header"][4] == last + 1 and W.REF_WALK.walk(mp, cam, 0, N + 1)["header"][4] == n_cells
    i_full, i_cut, i_rest = 4, len(steps) - 2, len(steps) - 1

    def extra(outs):
        f, a, b = (outs[i] for i in (i_full, i_cut, i_rest))
        Va, Ma, Vb, Mb = a["d_header"][2], a["d_header"][3], b["d_header"][2], b["d_header"][3]
        assert Va + Vb == f["d_header"][2] and Ma + Mb == f["d_header"][3] and Va > 0 and Vb > 0
        for k in ("d_visit_point", "d_visit_cell"):
            assert np.array_equal(np.concatenate([a[k][:Va], b[k][:Vb]]), f[k][:Va + Vb]), k
        tb = b["d_visit_trial"][:Vb]
        assert np.array_equal(np.concatenate([a["d_visit_trial"][:Va], np.where(tb >= 0, tb + Ma, -1)]), f["d_visit_trial"][:Va + Vb])
        for k in ("d_trial_obs_begin", "d_trial_cell", "d_trial_pos"):
            assert np.array_equal(np.concatenate([a[k][:Ma], b[k][:Mb]]), f[k][:Ma + Mb]), k
    return steps, {"N": N}, extra


def _capacities(cam, rng):
    mp = _copy(random_map(cam, n_kfs=8, n_points=300, n_candidates=200, seed=int(rng.integers(1 << 30))))
    w = W.REF_WALK.walk(mp, cam)
    V, M = int(w["header"][2]), int(w["header"][3])
    assert 0 < M < V
    return [Step(mp, max_visits=v, max_trials=t, label=f"max_visits {v}, max_trials {t}") for v, t in ((V, M), (V - 1, M), (V, M - 1), (V - 1, M - 1))], {}


def _patch_moves_first_meeting(cam, rng):
    T = _poses(rng, 11, 10)
    m = _Map(cam, T, 10, _ranks(T, 10, 6), rng)
    for x in _plane(cam, rng, 400, frac=1.0):
        m.point(x, rng.choice([2, 3]), rng.permutation(10)[:int(rng.integers(2, 6))])
    for i, x in enumerate(_plane(cam, rng, 150, frac=1.0)):
        m.candidate(x, i, rng.integers(10))
    mp0 = m.build()
    mp1 = _copy(mp0)
    meet0 = _first_meetings(mp0)
    # records rewritten: the record a point was first met through goes to a keyframe without overlap, or leaves every fts_
    movers = rng.permutation(np.flatnonzero(meet0 >= 0))[:120]
    far = np.flatnonzero(mp0["kf_rank"][:10] < 0)
    for i, p in enumerate(movers):
        o = meet0[p]
        if i % 2:
            f = int(rng.choice(far))
            mp1["obs_frame"][o], mp1["obs_order"][o] = f, m.slot(f)
        else:
            mp1["obs_order"][o] = -1
    dead = rng.permutation(np.flatnonzero(mp0["type"] >= 1))[:30]
    mp1["type"][dead] = 0
    promoted = np.setdiff1d(np.flatnonzero(mp0["type"] == 2), dead)[:30]
    mp1["type"][promoted] = 3
    moved = rng.permutation(550)[:40]
    mp1["pos"][moved] += rng.normal(0, 0.02, (40, 3))
    touched_obs = np.sort(meet0[movers]).astype(np.int32)
    touched = np.unique(np.concatenate([dead, promoted, moved])).astype(np.int32)
    meet1 = _first_meetings(mp1)
    frame_of = lambda mp, meet, p: int(mp["obs_frame"][meet[p]]) if meet[p] >= 0 else -1
    changed = sum(1 for p in movers if frame_of(mp0, meet0, p) != frame_of(mp1, meet1, p) and meet1[p] >= 0)
    lost = sum(1 for p in movers if meet1[p] < 0)
    w0, w1 = W.REF_WALK.walk(mp0, cam), W.REF_WALK.walk(mp1, cam)
    assert changed >= 40 and lost >= 3 and not np.array_equal(w0["kf_count"], w1["kf_count"]), (changed, lost)
    assert ((w0["point_cell"] >= -1) & (w1["point_cell"] == -2)).sum() >= 20
    return [Step(mp0, label="before"), Step(mp1, touched=touched, touched_obs=touched_obs, label="after the patch")], {"changed": changed, "lost": lost}


@functools.lru_cache(None)
def case(name, kind="pinhole"):
    cam = camera_models()[kind]
    rng = fuzz_rng(700 + CASE_NAMES.index(name))
    extra = None
    if name == "many_views":
        steps, facts = _many_views(cam, rng, kind)
    elif name in ("cell_limit", "exact_edges"):
        cam, steps, facts = globals()["_" + name](cam, rng)
    elif name == "cuts":
        steps, facts, extra = _cuts(cam, rng)
    else:
        steps, facts = globals()["_" + name](cam, rng)
    c = Case(name, kind, cam, steps, exact_px=name == "exact_edges", tied_cos=name == "close_view_ties", extra=extra, facts=facts)
    for s in steps:     # the builder conditions
        w = wanted(c, s)[0]
        assert s.mp["kf_rank"].max() < 16 and s.mp["obs_order"].max() < 4096 and s.mp["order"].max() < 65000
        assert c.exact_px or w["margin_px"] >= cc.CELL_MARGIN, (name, s.label, w["margin_px"])
        assert c.tied_cos or min(w["margin_cos"], w["margin_gap"]) >= COS_MARGIN, (name, s.label, w["margin_cos"], w["margin_gap"])
    return c


def wanted(c, step):
    """-> (the independent walk's answer, the oracle's) for a step, computed once"""
    if not hasattr(step, "_wanted"):
        step._wanted = (_walk(step, c.cam), oracle_reproject_map(step.mp, c.cam, step.first_cell, step.max_cells))
    return step._wanted


# ---- outputs: poisoned, between guard words ---------------------------------------------------------------------------------------
GUARD = 16           # elements of 0xA5 bytes on either side of every output
POISON = 0x55555555


def output_shapes(P, n_frames, max_visits, max_trials):
    i, d = np.int32, np.float64
    return {"d_header": ((capi.REPROJ_HEADER,), i), "d_point_cell": ((P,), i), "d_point_px": ((P, 2), d), "d_kf_count": ((n_frames,), i),
            "d_visit_point": ((max_visits,), i), "d_visit_cell": ((max_visits,), i), "d_visit_trial": ((max_visits,), i),
            "d_trial_cur": ((max_trials,), i), "d_trial_pos": ((max_trials, 3), d), "d_trial_obs_begin": ((max_trials,), i),
            "d_trial_obs_end": ((max_trials,), i), "d_trial_cell": ((max_trials,), i), "d_trial_px": ((max_trials, 2), d)}


VISIT_KEYS = ("d_visit_point", "d_visit_cell", "d_visit_trial")
TRIAL_KEYS = ("d_trial_cur", "d_trial_pos", "d_trial_obs_begin", "d_trial_obs_end", "d_trial_cell", "d_trial_px")


class Outputs:
    """name -> raw bytes: guard band, poisoned payload, guard band.  A backend hands `raw` (or a device copy of it) to the entry at
    `offset(k)` and puts back what the call left."""

    def __init__(self, P, n_frames, max_visits, max_trials):
        self.shapes = output_shapes(P, n_frames, max_visits, max_trials)
        self.raw = {}
        for k, (shape, dt) in self.shapes.items():
            raw = np.full((int(np.prod(shape)) + 2 * GUARD) * np.dtype(dt).itemsize, 0xA5, np.uint8)
            self.raw[k] = raw
            self[k][...] = np.nan if dt == np.float64 else POISON

    def offset(self, k):
        return GUARD * np.dtype(self.shapes[k][1]).itemsize

    def __getitem__(self, k):
        shape, dt = self.shapes[k]
        return self.raw[k].view(dt)[GUARD:GUARD + int(np.prod(shape))].reshape(shape)

    def guards_intact(self):
        for k, raw in self.raw.items():
            g = self.offset(k)
            assert (raw[:g] == 0xA5).all() and (raw[len(raw) - g:] == 0xA5).all(), k
        return True

    def untouched(self, k, start=0):
        v = self[k][start:]
        return bool(np.isnan(v).all() if v.dtype == np.float64 else (v == POISON).all())

    def struct(self, base):
        """svo_hip_reprojection with base[k] the address of raw[k] (host or device)"""
        return capi.Reprojection(*[base[n] + self.offset(n) for n, _ in capi.Reprojection._fields_])


def outputs_for(step):
    return Outputs(step.mp["pos"].shape[0], step.mp["T"].shape[0], step.max_visits, step.max_trials)


# ---- the rule ----------------------------------------------------------------------------------------------------------------
INTEGER_KEYS = ("point_cell", "kf_count", "visit_point", "visit_cell", "visit_trial", "trial_obs", "trial_cell")


def same_integers(a, b, what):
    assert [int(x) for x in a["header"][:5]] == [int(x) for x in b["header"][:5]], (what, a["header"], b["header"])
    for k in INTEGER_KEYS:
        assert np.array_equal(a[k], b[k]), (what, k)


def check_answer(c, step, got, px_tol_oracle):
    """got: a dict like the walk's (what a mutant, the oracle or a backend says about an unlimited call) against the walk and the
    oracle: integers identical, trial_pos bit for bit, pixels within the two bounds -> (largest px difference to the oracle, to the walk)"""
    w, o = wanted(c, step)
    same_integers(w, o, "walk vs oracle")
    same_integers(got, w, "against the walk")
    same_integers(got, o, "against the oracle")
    assert np.array_equal(np.asarray(got["trial_pos"]).view(np.uint64), w["trial_pos"].view(np.uint64))
    assert np.array_equal(o["trial_pos"].view(np.uint64), w["trial_pos"].view(np.uint64))
    seen = w["point_cell"] >= -1
    d_o = d_w = 0.0
    for key, rows in (("point_px", seen), ("trial_px", slice(None))):
        g, ow, ww = np.asarray(got[key])[rows], o[key][rows], w[key][rows]
        if g.size:
            eo, ew = np.abs(g - ow), np.abs(g - ww)
            assert (eo <= px_tol_oracle).all(), (key, "oracle", float(eo.max()))
            assert (ew <= cc.PIXEL_ATOL + cc.PIXEL_RTOL * np.abs(ww)).all(), (key, "walk", float(ew.max()))
            d_o, d_w = max(d_o, float(eo.max())), max(d_w, float(ew.max()))
    assert np.isnan(np.asarray(got["point_px"])[~seen]).all()      # defined only where the point was projected
    return d_o, d_w


def check_step(c, step, out, px_tol_oracle):
    """out: the Outputs a backend's call left -> (largest px difference to the oracle, to the walk)"""
    w, _ = wanted(c, step)
    assert out.guards_intact()
    h = [int(x) for x in out["d_header"]]
    E, V, M, end = (int(x) for x in w["header"][1:5])
    refused = E > MAX_IN_FRAME or V > step.max_visits or M > step.max_trials
    got = dict(header=np.array([0, E, V, M, end, 0, 0, 0], np.int32), point_cell=out["d_point_cell"], point_px=out["d_point_px"],
               kf_count=w["kf_count"] if E > MAX_IN_FRAME else out["d_kf_count"])
    if refused:
        assert h[:5] == [1, E, 0, 0, step.first_cell], h
        for k in VISIT_KEYS + TRIAL_KEYS:
            assert out.untouched(k), k
        for k in INTEGER_KEYS[2:] + ("trial_px", "trial_pos"):
            got[k] = w[k]
        return check_answer(c, step, got, px_tol_oracle)
    assert h == [0, E, V, M, end, 0, 0, 0], (h, [E, V, M, end])
    for k in VISIT_KEYS:
        got[k[2:]] = out[k][:V]
        assert out.untouched(k, V), k
    for k in TRIAL_KEYS:
        assert out.untouched(k, M), k
    got.update(trial_obs=out["d_trial_obs_begin"][:M], trial_cell=out["d_trial_cell"][:M], trial_px=out["d_trial_px"][:M], trial_pos=out["d_trial_pos"][:M])
    assert np.array_equal(out["d_trial_obs_end"][:M], out["d_trial_obs_begin"][:M] + 1)
    assert (out["d_trial_cur"][:M] == step.mp["cur"]).all()
    return check_answer(c, step, got, px_tol_oracle)


def check_case(c, outs, px_tol_oracle):
    """every step of a case under the rule, then what the case asserts across its steps -> the largest px differences"""
    d = [check_step(c, s, o, px_tol_oracle) for s, o in zip(c.steps, outs)]
    if c.extra is not None:
        c.extra(outs)
    return max(x for x, _ in d), max(x for _, x in d)


# ---- what a backend uploads ------------------------------------------------------------------------------------------------------
MAP_COLUMNS = (("pos", np.float64, 3), ("type", np.int32, 1), ("order", np.int32, 1), ("obs_begin", np.int32, 1), ("obs_count", np.int32, 1))
OBS_COLUMNS = (("obs_frame", np.int32, 1), ("obs_order", np.int32, 1), ("obs_level", np.int32, 1), ("obs_type", np.uint8, 1), ("obs_px", np.float64, 2),
               ("obs_f", np.float64, 3), ("obs_grad", np.float64, 2))


def patch_of(step):
    """-> (index, {column: rows}, obs_index, {column: rows}) of the step's patch: the whole map for a new mirror"""
    mp = step.mp
    idx = np.arange(mp["pos"].shape[0], dtype=np.int32) if step.touched is None else np.asarray(step.touched, np.int32)
    oidx = np.arange(mp["obs_frame"].shape[0], dtype=np.int32) if step.touched is None else np.asarray(step.touched_obs, np.int32)
    return (idx, {k: np.ascontiguousarray(mp[k][idx], dt) for k, dt, _ in MAP_COLUMNS}, oidx,
            {k: np.ascontiguousarray(mp[k][oidx], dt) for k, dt, _ in OBS_COLUMNS})


# ---- the entry's argument checks ---------------------------------------------------------------------------------------------
def _null(key):
    return lambda c: c.__setitem__(key, None)


def _put(key, value):
    return lambda c: c.__setitem__(key, value(c) if callable(value) else value)


def _field(key, name, value):
    def change(c):
        obj = c[key]
        for part in name.split(".")[:-1]:
            obj = getattr(obj, part)
        setattr(obj, name.split(".")[-1], value(c) if callable(value) else value)
    return change


# (label, change to a valid call, the code csrc/map_mirror.hip states).  A call is a dict: cam, frames, cur_frame, d_kf_rank, map,
# patch, grid, first_cell, max_cells_with_trials, max_visits, max_trials, out -- structs of rpg_svo_amd.capi, addresses and ints.
ARG_ROWS = [(f"NULL {k}", _null(k), EINVAL) for k in ("cam", "frames", "map", "grid", "out", "d_kf_rank")] + [
    ("n_frames 0", _field("frames", "n_frames", 0), EINVAL),
    ("n_frames 65", _field("frames", "n_frames", 65), EINVAL),
    ("cur_frame -1", _put("cur_frame", -1), EINVAL),
    ("cur_frame n_frames", _put("cur_frame", lambda c: c["frames"].n_frames), EINVAL),
    ("NULL frames.d_T_f_w", _field("frames", "d_T_f_w", None), EINVAL),
    ("n_points 8193", _field("map", "n_points", 8193), ERANGE),
    ("n_points -1", _field("map", "n_points", -1), ERANGE),
    ("n_cells 2049", _field("grid", "n_cells", 2049), ERANGE),
    ("n_cells 0", _field("grid", "n_cells", 0), EINVAL),
    ("cell_size 0", _field("grid", "cell_size", 0), EINVAL),
    ("NULL grid.d_cell_rank", _field("grid", "d_cell_rank", None), EINVAL),
    ("first_cell -1", _put("first_cell", -1), EINVAL),
    ("first_cell n_cells + 1", _put("first_cell", lambda c: c["grid"].n_cells + 1), EINVAL),
    ("max_visits -1", _put("max_visits", -1), EINVAL),
    ("max_trials -1", _put("max_trials", -1), EINVAL),
    ("NULL map.d_pos", _field("map", "d_pos", None), EINVAL),
    ("NULL map.d_obs_order", _field("map", "d_obs_order", None), EINVAL),
    ("NULL out.d_header", _field("out", "d_header", None), EINVAL),
    ("NULL out.d_point_px", _field("out", "d_point_px", None), EINVAL),
    ("NULL out.d_visit_trial with max_visits > 0", _field("out", "d_visit_trial", None), EINVAL),
    ("NULL out.d_trial_px with max_trials > 0", _field("out", "d_trial_px", None), EINVAL),
    ("patch n_points -1", _field("patch", "n_points", -1), EINVAL),
    ("patch n_obs -1", _field("patch", "n_obs", -1), EINVAL),
    ("patch NULL d_pos", _field("patch", "d_pos", None), EINVAL),
    ("patch NULL d_obs_order", _field("patch", "d_obs_order", None), EINVAL),
    ("patch NULL obs.d_px", _field("patch", "obs.d_px", None), EINVAL),
]
CALL_ORDER = ("cam", "frames", "cur_frame", "d_kf_rank", "map", "patch", "grid", "first_cell", "max_cells_with_trials", "max_visits", "max_trials", "out")


def invoke(lib, call, stream=None):
    a = [C.byref(v) if isinstance(v, C.Structure) else C.c_void_p(v) if k == "d_kf_rank" else None if v is None else C.c_int(v)
         for k, v in ((k, call[k]) for k in CALL_ORDER)]
    lib.svo_hip_reproject_map.restype = C.c_int
    return lib.svo_hip_reproject_map(*a, C.c_void_p(stream) if stream else None)


@functools.lru_cache(None)
def args_step():
    """a small valid call for the argument table: 40 points, 10 candidates"""
    cam = camera_models()["pinhole"]
    return cam, Step(_copy(random_map(cam, n_kfs=4, n_points=40, n_candidates=10, seed=3, n_overlap=3)))


def empty_maps():
    """maps on which the call succeeds with E = V = M = 0: no entries at all; entries, all of them dead"""
    cam, s = args_step()
    none = _copy(s.mp)
    for k, _, _ in MAP_COLUMNS:
        none[k] = none[k][:0]
    for k, _, _ in OBS_COLUMNS:
        none[k] = none[k][:0]
    dead = _copy(s.mp)
    dead["type"][:] = 0
    return cam, [Step(none, label="n_points 0"), Step(dead, label="no point and no candidate alive")]


def check_empty(step, out):
    assert out.guards_intact()
    assert [int(x) for x in out["d_header"]] == [0, 0, 0, 0, step.mp["n_cols"] * step.mp["n_rows"], 0, 0, 0]
    assert (out["d_point_cell"] == -2).all() and out.untouched("d_point_px") and (out["d_kf_count"] == 0).all()
    for k in VISIT_KEYS + TRIAL_KEYS:
        assert out.untouched(k), k


# ---- the stand-alone sanitizer program's files (tests/host/map_mirror_asan_main.cpp) -------------------------------------------
def write_steps(path, items):
    """items: [(cam, Step)].  Little-endian: i32 count, then per step 14 i32, 9 f64 and the arrays in the order read below"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(items)))
        for cam, s in items:
            mp = s.mp
            P, O, n_frames = mp["pos"].shape[0], mp["obs_frame"].shape[0], mp["T"].shape[0]
            f.write(struct.pack("<14i", int(getattr(cam, "model", 0)), cam.width, cam.height, n_frames, mp["cur"], P, O, mp["cell_size"], mp["n_cols"],
                                mp["n_rows"], s.first_cell, min(s.max_cells, 1 << 30), s.max_visits, s.max_trials))
            f.write(struct.pack("<9d", cam.fx, cam.fy, cam.cx, cam.cy, *tuple(getattr(cam, "d", (0.0,) * 5))))
            for a, dt in ((mp["T"], np.float64), (mp["kf_rank"], np.int32), (mp["pos"], np.float64), (mp["type"], np.int32), (mp["order"], np.int32),
                          (mp["obs_begin"], np.int32), (mp["obs_count"], np.int32), (mp["obs_frame"], np.int32), (mp["obs_order"], np.int32),
                          (mp["obs_level"], np.int32), (mp["obs_type"], np.int32), (mp["obs_px"], np.float64), (mp["obs_f"], np.float64),
                          (mp["obs_grad"], np.float64), (mp["cell_rank"], np.int32)):
                f.write(np.ascontiguousarray(a, dt).tobytes())


def read_outputs(path, items):
    """-> [Outputs] as the program's calls left them (it allocates every array at exactly its size and poisons it the same way)"""
    outs = []
    with open(path, "rb") as f:
        for _, s in items:
            assert struct.unpack("<i", f.read(4))[0] == OK
            out = outputs_for(s)
            for k, (shape, dt) in out.shapes.items():
                out[k][...] = np.frombuffer(f.read(int(np.prod(shape)) * np.dtype(dt).itemsize), dt).reshape(shape)
            outs.append(out)
        assert f.read() == b""
    return outs


def check_arguments(lib, make_call, px_tol_oracle, stream=None):
    """every row of ARG_ROWS returns its code and leaves the poisoned outputs untouched; the unspoilt call and the two empty maps
    succeed.  make_call(cam, step) -> (call, fetch)"""
    cam, s = args_step()
    for label, change, code in ARG_ROWS:
        call, fetch = make_call(cam, s)
        change(call)
        assert invoke(lib, call, stream) == code, label
        out = fetch()
        assert out.guards_intact() and all(out.untouched(k) for k in out.shapes), label
    call, fetch = make_call(cam, s)
    assert invoke(lib, call, stream) == OK
    c = Case("arguments", "pinhole", cam, [s])
    check_step(c, s, fetch(), px_tol_oracle)
    for e in empty_maps()[1]:
        call, fetch = make_call(cam, e)
        assert invoke(lib, call, stream) == OK, e.label
        check_empty(e, fetch())
