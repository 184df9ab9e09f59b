"""TEST INFRASTRUCTURE, not a test.  Reprojector::reprojectMap up to the first findMatchDirect, written a third time -- from
the reference's text (svo/src/reprojector.cpp:64-142, 151-153, 206-217; Point::getCloseViewObs, svo/src/point.cpp:97-117), in
plain Python over the plain-array map of helpers.random_map, and NOT by translating oracle/svo_oracle_track.c or
rpg_svo_amd/csrc/map_mirror.hip.  Nothing of `oracle` or of the library under test is imported here.

  * the keyframes with overlap, closest first (:76-84); every Feature of a keyframe in fts_ order (:90); a point is projected
    only once (:97-100); reprojectPoint pushes it to the back of its cell's list (:206-217) and credits the keyframe (:101-102);
  * the candidates afterwards, in list order (:108-123);
  * the cells in grid_.cell_order (:132-136); inside a cell `list::sort` with "lhs.type_ > rhs.type_" (:144-153) -- stable,
    like sorted();
  * getCloseViewObs for every point of a visited cell: `cos_angle > min_cos_angle` from 0 (strict: the first of equal
    cosines stays, and with no positive cosine the first observation), `min_cos_angle < 0.5` -> no view;
  * what the batched drop-in adds: the walk starts at `first_cell` and ends right after the cell that brings the number of
    cells with a trial to `max_cells_with_trials`.

Projection, border and cell come from camera_reference.REF (mpmath, 40 digits); the frame positions -R^T t and the cosines
of the viewing directions are computed in mpmath here.  Two cosines (or a cosine and 0.5) that differ by less than 1e-30 are
equal: the computation is good to 1e-38, so this is exact equality of the real numbers for every input a case builder makes.

walk() returns what helpers.oracle_reproject_map returns, and per kind of decision its smallest margin over the map:
`margin_px` (px to the nearest frame border or cell edge that decides a cell), `margin_cos` (|cos - 0.5| of a binned point's
best cosine), `margin_gap` (best cosine minus the best cosine of another frame, or minus 0, whichever is nearer); per point
they are in `geometry`.

`Walk` is a class so that tests/test_map_mirror_rules.py can judge the comparison rule with mutants (one member each).
`literal_walk` is the older restatement tests/test_map_mirror.py holds the oracle against: the same loops through a
`reproject_point` of the caller's choice, without the close-view step."""
import numpy as np

import camera_reference as cr
from camera_reference import M, REF, mpf

EQUAL = mpf("1e-30")
HALF = mpf("0.5")
INF = float("inf")


def literal_walk(mp, reproject_point):
    """reproject_point(p) -> cell or -1.  -> point_cell [P], kf_count [n_frames], [(point, visiting rank of its cell)]"""
    P = mp["pos"].shape[0]
    n_frames = mp["T"].shape[0]
    cells = [[] for _ in range(mp["n_cols"] * mp["n_rows"])]
    kf_count = np.zeros(n_frames, dtype=np.int32)
    last_projected = np.zeros(P, dtype=bool)
    point_cell = np.full(P, -2, dtype=np.int32)

    def reproject(p):
        k = reproject_point(p)
        point_cell[p] = k
        if k >= 0:
            cells[k].append(p)
        return k >= 0

    for rank in range(n_frames):
        fs = np.nonzero(mp["kf_rank"] == rank)[0]
        if fs.size == 0:
            continue
        f = int(fs[0])
        fts = []   # the keyframe's fts_: (position, point)
        for p in range(P):
            if mp["type"][p] < 2:
                continue
            for o in range(mp["obs_begin"][p], mp["obs_begin"][p] + mp["obs_count"][p]):
                if mp["obs_frame"][o] == f and mp["obs_order"][o] >= 0:
                    fts.append((int(mp["obs_order"][o]), p))
        for _, p in sorted(fts):
            if last_projected[p]:
                continue
            last_projected[p] = True
            if reproject(p):
                kf_count[f] += 1
    cands = sorted((int(mp["order"][p]), p) for p in range(P) if mp["type"][p] == 1)
    for _, p in cands:
        reproject(p)
    cell_of_rank = np.argsort(mp["cell_rank"])
    visit = []
    for i in range(len(cells)):
        cell = sorted(cells[cell_of_rank[i]], key=lambda p: -mp["type"][p])  # list::sort is stable, so is sorted()
        visit += [(p, i) for p in cell]
    return point_cell, kf_count, visit


# ---- the arithmetic: one pass per map, shared by every walk over it (the mutants change decisions, not numbers) ---------------
def frame_positions(T):
    """Frame::pos() = -R^T t of every row of the frame table, in mpmath"""
    out = []
    for row in T:
        t = [mpf(float(v)) for v in row]
        out.append(tuple(-(t[i] * t[9] + t[3 + i] * t[10] + t[6 + i] * t[11]) for i in range(3)))
    return out


def _unit(v):
    n = M.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return (v[0] / n, v[1] / n, v[2] / n)


def cell_margin(cam, cell_size, cell, u, v):
    """px from the nearest boundary that decides the cell: inside the frame the four borders and the cell's edges, outside the
    border violated by the most"""
    lo, hi_u, hi_v = cr.FRAME_BORDER, cam.width - cr.FRAME_BORDER, cam.height - cr.FRAME_BORDER
    if cell >= 0:
        inside = [u - lo, hi_u - u, v - lo, hi_v - v]
        grid = [t - cell_size * M.floor(t / cell_size) for t in (u, v)]
        return float(min(inside + grid + [cell_size - g for g in grid]))
    return float(max(lo - u, u - hi_u, lo - v, v - hi_v))


class Geometry:
    """per live entry (type >= 1): cell, pixel, depth in the current frame, margin; per binned entry with observations: the
    cosine of every record's viewing direction.  Computed on demand and kept."""

    def __init__(self, mp, cam):
        self.mp, self.cam, self.c = mp, cam, cr.Cam(cam)
        self.fpos = frame_positions(mp["T"])
        self.T_cur = mp["T"][mp["cur"]]
        self._proj, self._cos = {}, {}

    def project(self, p):
        """-> (cell or -1, (u, v) as mpf, depth in the current frame, margin in px)"""
        if p not in self._proj:
            mp = self.mp
            q = REF.transform(self.T_cur, mp["pos"][p])
            assert q[2] != 0, ("a point at depth 0 in the current frame: the reference divides by it", p)
            cell, (u, v) = REF.reproject_point(self.c, self.T_cur, mp["pos"][p], mp["cell_size"], mp["n_cols"])
            self._proj[p] = (cell, (u, v), q[2], cell_margin(self.cam, mp["cell_size"], cell, u, v))
        return self._proj[p]

    def cosines(self, p):
        """the cosine between the current frame's and each record's viewing direction of point p, in record order"""
        if p not in self._cos:
            mp = self.mp
            x = [mpf(float(v)) for v in mp["pos"][p]]
            cur = self.fpos[mp["cur"]]
            obs_dir = _unit([cur[i] - x[i] for i in range(3)])
            out = []
            for o in range(mp["obs_begin"][p], mp["obs_begin"][p] + mp["obs_count"][p]):
                fp = self.fpos[int(mp["obs_frame"][o])]
                d = _unit([fp[i] - x[i] for i in range(3)])
                out.append(obs_dir[0] * d[0] + obs_dir[1] * d[1] + obs_dir[2] * d[2])
            self._cos[p] = out
        return self._cos[p]

    def inherit(self, other, same, moved=()):
        """takes over what `other` (the Geometry of a map with the same frames and camera) has computed: for the entries `same`,
        unchanged in position and records, everything; for (p, q) in `moved`, entry p now at entry q's position, q's projection"""
        for p in same:
            if p in other._proj:
                self._proj[p] = other._proj[p]
            if p in other._cos:
                self._cos[p] = other._cos[p]
        for p, q in moved:
            if q in other._proj:
                self._proj[p] = other._proj[q]


def geometry(mp, cam):
    """the Geometry of a map, kept on the map itself (a builder that changes a map's arrays makes a new dict)"""
    if "_geometry" not in mp:
        mp["_geometry"] = Geometry(mp, cam)
    return mp["_geometry"]


# ---- the walk ----------------------------------------------------------------------------------------------------------------
class Walk:
    def records(self, mp, p):
        return range(int(mp["obs_begin"][p]), int(mp["obs_begin"][p]) + int(mp["obs_count"][p]))

    def meeting_records(self, mp, p):
        """the observation records through which a keyframe's fts_ can lead to point p"""
        return self.records(mp, p)

    def keyframe_features(self, mp):
        """(keyframe, point) in the order the keyframe loop meets them: keyframes closest first, each one's fts_ in list order"""
        n_frames = mp["T"].shape[0]
        fts = [[] for _ in range(n_frames)]
        for p in range(mp["pos"].shape[0]):
            if mp["type"][p] < 2:   # (*it_ftr)->point of a keyframe's feature is a live UNKNOWN / GOOD point
                continue
            for o in self.meeting_records(mp, p):
                if mp["obs_order"][o] >= 0:
                    fts[int(mp["obs_frame"][o])].append((int(mp["obs_order"][o]), p))
        close_kfs = sorted((int(r), f) for f, r in enumerate(mp["kf_rank"]) if r >= 0)
        for _, f in close_kfs:
            for _, p in sorted(fts[f]):
                yield f, p

    def candidates(self, mp):
        """MapPointCandidates::candidates_ in list order"""
        return [p for _, p in sorted((int(mp["order"][p]), p) for p in range(mp["pos"].shape[0]) if mp["type"][p] == 1)]

    def in_front(self, depth):
        return True   # reprojectPoint has no test of the depth

    def credited(self, mp, f, p):
        """the keyframes whose counter a projected point raises: the one whose feature led to it"""
        return [f]

    def sort_cell(self, mp, cell):
        """cell: [(binning number, point)] in push_back order -> the points as reprojectCell walks them"""
        return [p for _, p in sorted(cell, key=lambda e: -int(mp["type"][e[1]]))]

    def view_records(self, mp, p):
        """the observations getCloseViewObs looks at: obs_, every one"""
        return list(self.records(mp, p))

    def better(self, cos, best):
        return cos > best + EQUAL

    def close(self, best_cos):
        return not best_cos < HALF - EQUAL

    def counts_for_the_cut(self, n_visits, n_trials):
        return n_trials > 0

    cut_slack = 0   # cells walked beyond the one that reaches the maximum

    def close_view(self, mp, geo, p):
        """-> (record or -1, has a close view, |cos - 0.5|, gap)"""
        recs = self.view_records(mp, p)
        if not recs:
            return -1, False, INF, INF
        o0 = int(mp["obs_begin"][p])
        cos = geo.cosines(p)
        best, min_cos_angle = recs[0], mpf(0)
        for o in recs:
            if self.better(cos[o - o0], min_cos_angle):
                min_cos_angle, best = cos[o - o0], o
        frame_of = lambda o: int(mp["obs_frame"][o])
        others = [cos[o - o0] for o in recs if frame_of(o) != frame_of(best)] if min_cos_angle > 0 else []
        top = max([cos[o - o0] for o in recs])
        gap = float(min_cos_angle - max(others + [mpf(0)])) if min_cos_angle > 0 else float(-top)
        return best, self.close(min_cos_angle), float(abs(min_cos_angle - HALF)), gap

    def walk(self, mp, cam, first_cell=0, max_cells_with_trials=1 << 30):
        geo = geometry(mp, cam)
        P, n_frames, n_cells = mp["pos"].shape[0], mp["T"].shape[0], mp["n_cols"] * mp["n_rows"]
        cells = [[] for _ in range(n_cells)]
        point_cell = np.full(P, -2, np.int32)
        point_px = np.full((P, 2), np.nan)
        kf_count = np.zeros(n_frames, np.int32)
        margin_px, n_binned = INF, 0

        def reproject_point(p):
            nonlocal margin_px, n_binned
            cell, (u, v), depth, margin = geo.project(p)
            point_px[p] = float(u), float(v)
            margin_px = min(margin_px, margin)
            if cell >= 0 and self.in_front(depth):
                cells[cell].append((n_binned, p))
                n_binned += 1
                point_cell[p] = cell
                return True
            point_cell[p] = -1
            return False

        projected = set()
        for f, p in self.keyframe_features(mp):
            if p in projected:
                continue
            projected.add(p)
            if reproject_point(p):
                for g in self.credited(mp, f, p):
                    kf_count[g] += 1
        for p in self.candidates(mp):
            reproject_point(p)

        cell_of_rank = np.argsort(mp["cell_rank"], kind="stable")
        visit_point, visit_cell, visit_trial, trial_obs, trial_cell = [], [], [], [], []
        margin_cos = margin_gap = INF
        cells_with_trials, i, slack = 0, first_cell, self.cut_slack
        while i < n_cells and (cells_with_trials < max_cells_with_trials or slack > 0):
            if cells_with_trials >= max_cells_with_trials:
                slack -= 1
            n_visits = n_trials = 0
            for p in self.sort_cell(mp, cells[cell_of_rank[i]]):
                best, close, d_half, gap = self.close_view(mp, geo, p)
                margin_cos, margin_gap = min(margin_cos, d_half), min(margin_gap, gap)
                visit_point.append(p)
                visit_cell.append(i)
                n_visits += 1
                if close:
                    visit_trial.append(len(trial_obs))
                    trial_obs.append(best)
                    trial_cell.append(i)
                    n_trials += 1
                else:
                    visit_trial.append(-1)
            if self.counts_for_the_cut(n_visits, n_trials) and cells_with_trials < max_cells_with_trials:
                cells_with_trials += 1
            i += 1
        a = lambda v: np.array(v, np.int32)
        V, Mt = len(visit_point), len(trial_obs)
        trial_point = [p for p, t in zip(visit_point, visit_trial) if t >= 0]
        header = np.zeros(8, np.int32)
        header[:5] = 0, n_binned, V, Mt, i
        return dict(header=header, point_cell=point_cell, point_px=point_px, kf_count=kf_count, visit_point=a(visit_point),
                    visit_cell=a(visit_cell), visit_trial=a(visit_trial), trial_obs=a(trial_obs), trial_cell=a(trial_cell),
                    trial_px=point_px[trial_point].reshape(Mt, 2), trial_pos=np.asarray(mp["pos"], np.float64)[trial_point].reshape(Mt, 3),
                    margin_px=margin_px, margin_cos=margin_cos, margin_gap=margin_gap)


REF_WALK = Walk()


# ---- mutants: each a plausible slip of a kernel that orders by keys and fetches records in batches of eight -------------------
class FirstEightMeet(Walk):
    """only the first eight records of a point can be its first meeting"""
    def meeting_records(self, mp, p):
        return list(self.records(mp, p))[:8]


class FirstEightView(Walk):
    """only the first eight records of a point are looked at for the close view"""
    def view_records(self, mp, p):
        return list(self.records(mp, p))[:8]


class MeetByPosition(Walk):
    """first meeting by the smallest fts_ position, whatever the keyframe's rank"""
    def keyframe_features(self, mp):
        rank = mp["kf_rank"]
        fts = []
        for p in range(mp["pos"].shape[0]):
            if mp["type"][p] < 2:
                continue
            for o in self.records(mp, p):
                f = int(mp["obs_frame"][o])
                if mp["obs_order"][o] >= 0 and rank[f] >= 0:
                    fts.append((int(mp["obs_order"][o]), int(rank[f]), f, p))
        for _, _, f, p in sorted(fts):
            yield f, p


class ViewFromOverlapOnly(Walk):
    """the close view ignores observations in keyframes without overlap"""
    def view_records(self, mp, p):
        recs = [o for o in self.records(mp, p) if mp["kf_rank"][int(mp["obs_frame"][o])] >= 0]
        return recs or list(self.records(mp, p))[:1]


class LastTieWins(Walk):
    """`>=`: of equal cosines the last record is taken"""
    def better(self, cos, best):
        return cos >= best - EQUAL


class StrictHalf(Walk):
    """cos > 0.5 required; the reference accepts 0.5"""
    def close(self, best_cos):
        return best_cos > HALF + EQUAL


class TypeAscending(Walk):
    def sort_cell(self, mp, cell):
        return [p for _, p in sorted(cell, key=lambda e: int(mp["type"][e[1]]))]


class EntryOrderInCell(Walk):
    """equal types in entry order, not in binning order"""
    def sort_cell(self, mp, cell):
        return [p for _, p in sorted(cell, key=lambda e: (-int(mp["type"][e[1]]), e[1]))]


class CandidatesInEntryOrder(Walk):
    def candidates(self, mp):
        return [p for p in range(mp["pos"].shape[0]) if mp["type"][p] == 1]


class DepthTest(Walk):
    """a point behind the camera is dropped"""
    def in_front(self, depth):
        return depth > 0


class CreditEveryObserver(Walk):
    """kf_count raised for every overlapping keyframe that has the point in its fts_"""
    def credited(self, mp, f, p):
        return sorted({int(mp["obs_frame"][o]) for o in self.records(mp, p)
                       if mp["obs_order"][o] >= 0 and mp["kf_rank"][int(mp["obs_frame"][o])] >= 0})


class CutCountsVisits(Walk):
    """the cut counts cells with a visit, not cells with a trial"""
    def counts_for_the_cut(self, n_visits, n_trials):
        return n_visits > 0


class CutOneLate(Walk):
    cut_slack = 1


MUTANTS = {
    "first eight records for the first meeting": FirstEightMeet,
    "first eight records for the close view": FirstEightView,
    "first meeting by position regardless of rank": MeetByPosition,
    "non-overlapping keyframes ignored in the close view": ViewFromOverlapOnly,
    "last record wins a cosine tie": LastTieWins,
    "cos > 0.5 required": StrictHalf,
    "type ascending": TypeAscending,
    "equal types in entry order": EntryOrderInCell,
    "candidates in entry order": CandidatesInEntryOrder,
    "a depth test": DepthTest,
    "kf_count to every overlapping observer": CreditEveryObserver,
    "the cut counts cells with visits": CutCountsVisits,
    "the cut stops one cell late": CutOneLate,
}
