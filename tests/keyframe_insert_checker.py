"""TEST INFRASTRUCTURE (numpy only).  svo_hip_keyframe_insert (K12, include/svo_hip.h) restated the way the reference does it:
small objects with Python lists -- Point.obs, Frame.fts, the candidates, the keyframes -- and the calls of
frame_handler_mono.cpp:196-200, 224-232 in their order: Point::addFrameRef (obs.insert(0, ..)), MapPointCandidates::
addCandidatePointToFrame, Map::safeDeleteFrame with removePtFrameRef / safeDeletePoint, Frame::removeKeyPoint / setKeyPoints /
checkKeyPoints as frame.cpp writes them, removeFrameCandidates, Map::addKeyframe.  Nothing here is shared with the kernel.

`insert(cam, state, inp)` takes the arrays of svo_hip_seq_map (a dict of numpy arrays, rpg_svo_amd.capi.SEQ_MAP_FIELDS) and of
svo_hip_keyframe_insert_in, builds the objects of every acting sequence, runs the steps and writes the objects back over a copy
of the arrays: what the call does not define (records beyond n_obs, rows beyond n_fts, the tables of untouched keyframes) keeps
its bytes.  A record's bytes beyond the list's end are what a shift in an array leaves there, so a Point keeps the array image
of its list (`image`) next to the list.

The rules for data that cannot index (a point index outside [0, P), a point of type 0, a record whose kf or row lies outside
its table, a kf_remove outside [0, n_kf), a second row with the point of an earlier one) are the header's, stated here once
more where they apply; the reference has no such case -- it would follow a dangling pointer.

`mutant` names one deliberate mistake (MUTANTS); tests/test_keyframe_insert_rules.py shows that the cases tell each from
the rule."""
import numpy as np

RESULT_IS_KEYFRAME = 1
DELETED, CANDIDATE, UNKNOWN, GOOD = 0, 1, 2, 3
STATE = ("n_kf", "kf_list", "kf_store_slot", "kf_T", "kf_n_fts", "kf_key_pts", "ftr_px", "ftr_f", "ftr_level", "ftr_point", "pt_pos", "pt_type",
         "pt_order", "pt_n_obs", "obs_kf", "obs_row", "obs_level", "obs_px", "obs_f")
INPUTS = ("result", "n", "px", "f", "level", "has_point", "ftr_point", "T_out", "slot", "key_pts", "kf_remove")
OUTPUTS = ("status", "kf_new_slot", "kf_removed_slot", "n_promoted", "n_points_deleted")
MUTANTS = ("push_back", "promote_before_frame_ref", "delete_at_one", "no_rescan", "rescan_from_null", "rescan_on_final_state",
           "appended_skipped", "remove_before_promote", "new_frame_at_front")


def state_shapes(B, K, F, P, R):
    """name -> (shape, numpy dtype) of svo_hip_seq_map's arrays"""
    i, d = np.int32, np.float64
    return dict(n_kf=((B,), i), kf_list=((B, K), i), kf_store_slot=((B * K,), i), kf_T=((B * K, 12), d), kf_n_fts=((B * K,), i),
                kf_key_pts=((B * K, 5), i), ftr_px=((B * K, F, 2), d), ftr_f=((B * K, F, 3), d), ftr_level=((B * K, F), i),
                ftr_point=((B * K, F), i), pt_pos=((B, P, 3), d), pt_type=((B, P), i), pt_order=((B, P), i), pt_n_obs=((B, P), i),
                obs_kf=((B, P, R), i), obs_row=((B, P, R), i), obs_level=((B, P, R), i), obs_px=((B, P, R, 2), d), obs_f=((B, P, R, 3), d))


def empty_state(B, K, F, P, R):
    s = {k: np.zeros(shape, dt) for k, (shape, dt) in state_shapes(B, K, F, P, R).items()}
    for k in ("kf_list", "kf_key_pts", "ftr_point", "obs_row"):
        s[k][...] = -1
    return s


class Overflow(Exception):
    pass


class Feature:
    """a row of a keyframe's table"""

    def __init__(self, frame, px, f, level, point, raw_point):
        self.frame, self.px, self.f, self.level, self.point, self.raw_point, self.written = frame, px, f, level, point, raw_point, False

    def set_point(self, point):
        self.point, self.written = point, True


class Record:
    """an element of Point::obs_: the columns it carries, and the Feature it is (a table row, or a Feature in no list)"""

    def __init__(self, kf, row, level, px, f, frame):
        self.kf, self.row, self.level, self.px, self.f, self.frame = kf, row, level, px, f, frame

    def feature(self):
        """the row of its keyframe's table that the record names, None where kf or row cannot index"""
        return self.frame.fts[self.row] if self.frame is not None and 0 <= self.row < len(self.frame.fts) else None


class Point:
    def __init__(self, index, type_, order, image):
        self.index, self.type, self.order, self.obs, self.image = index, type_, order, [], image

    def stored(self):
        """the list has changed: its array image follows, what lies beyond the end stays"""
        self.image[:len(self.obs)] = [(r.kf, r.row, r.level, r.px, r.f) for r in self.obs]


class Frame:
    def __init__(self, cam, slot, g):
        self.cam, self.slot, self.g = cam, slot, g
        self.fts, self.key_pts = [], [None] * 5
        self.key_pts_written = self.n_fts_written = False
        self.mutant, self.waiting = None, None

    # frame.cpp:67-70
    def addFeature(self, ftr, F):
        if len(self.fts) + 1 > F:
            raise Overflow
        self.fts.append(ftr)
        self.n_fts_written = True

    # frame.cpp:72-80
    def setKeyPoints(self):
        self.key_pts_written = True
        for i in range(5):
            if self.key_pts[i] is not None and (self.key_pts[i].point is None or self.mutant == "rescan_from_null"):
                self.key_pts[i] = None
        for ftr in self.fts:
            if ftr.point is not None:
                self.checkKeyPoints(ftr)

    # frame.cpp:82-126
    def checkKeyPoints(self, ftr):
        cu, cv = self.cam.width // 2, self.cam.height // 2
        kp = self.key_pts
        x, y = float(ftr.px[0]), float(ftr.px[1])
        far = lambda q: max(abs(float(q.px[0]) - cu), abs(float(q.px[1]) - cv))   # (max(a, b) is b when b > a, as std::max)
        area = lambda q: (float(q.px[0]) - cu) * (float(q.px[1]) - cv)
        if kp[0] is None:
            kp[0] = ftr
        elif far(ftr) < far(kp[0]):
            kp[0] = ftr
        for k, inside in ((1, x >= cu and y >= cv), (2, x >= cu and y < cv), (3, x < cv and y < cv), (4, x < cv and y >= cv)):
            if inside:
                if kp[k] is None:
                    kp[k] = ftr
                elif area(ftr) > area(kp[k]):
                    kp[k] = ftr

    # frame.cpp:128-139
    def removeKeyPoint(self, ftr):
        found = False
        for i in range(5):
            if self.key_pts[i] is ftr:
                self.key_pts[i] = None
                self.key_pts_written = True
                found = True
        if found:
            if self.mutant == "no_rescan":
                return
            if self.mutant == "rescan_on_final_state":
                if self not in self.waiting:
                    self.waiting.append(self)
                return
            self.setKeyPoints()


class SequenceObjects:
    """the objects of one sequence, built from the arrays and written back over them"""

    def __init__(self, cam, st, b, dims):
        K, F, P, R = dims
        self.cam, self.b, self.dims = cam, b, dims
        clamp = lambda v, hi: min(max(int(v), 0), hi)
        self.points = {}
        for p in range(P):
            if st["pt_type"][b, p] != DELETED:
                image = [(int(st["obs_kf"][b, p, r]), int(st["obs_row"][b, p, r]), int(st["obs_level"][b, p, r]), st["obs_px"][b, p, r].copy(),
                          st["obs_f"][b, p, r].copy()) for r in range(R)]
                self.points[p] = Point(p, int(st["pt_type"][b, p]), int(st["pt_order"][b, p]), image)
        self.frames = []
        for slot in range(K):
            g = b * K + slot
            fr = Frame(cam, slot, g)
            for row in range(clamp(st["kf_n_fts"][g], F)):
                raw = int(st["ftr_point"][g, row])
                fr.fts.append(Feature(fr, st["ftr_px"][g, row].copy(), st["ftr_f"][g, row].copy(), int(st["ftr_level"][g, row]), self.points.get(raw), raw))
            for k in range(5):
                row = int(st["kf_key_pts"][g, k])
                fr.key_pts[k] = fr.fts[row] if 0 <= row < len(fr.fts) else None
            self.frames.append(fr)
        for p, pt in self.points.items():
            for r in range(clamp(st["pt_n_obs"][b, p], R)):
                kf, row, level, px, f = pt.image[r]
                frame = self.frames[kf - b * K] if b * K <= kf < b * K + K else None
                pt.obs.append(Record(kf, row, level, px, f, frame))
        n_kf = clamp(st["n_kf"][b], K)
        self.kf_list = [int(s) for s in st["kf_list"][b, :n_kf]]

    def write_back(self, st):
        b, (K, F, P, R) = self.b, self.dims
        for p, pt in self.points.items():
            st["pt_type"][b, p], st["pt_n_obs"][b, p] = pt.type, len(pt.obs)
            for r, (kf, row, level, px, f) in enumerate(pt.image):
                st["obs_kf"][b, p, r], st["obs_row"][b, p, r], st["obs_level"][b, p, r] = kf, row, level
                st["obs_px"][b, p, r], st["obs_f"][b, p, r] = px, f
        for fr in self.frames:
            g = fr.g
            for row, ftr in enumerate(fr.fts):
                st["ftr_px"][g, row], st["ftr_f"][g, row], st["ftr_level"][g, row] = ftr.px, ftr.f, ftr.level
                if ftr.written:
                    st["ftr_point"][g, row] = -1 if ftr.point is None else ftr.point.index
            if fr.n_fts_written:
                st["kf_n_fts"][g] = 0 if fr.removed else len(fr.fts)
            if fr.key_pts_written:
                st["kf_key_pts"][g] = [-1 if q is None or fr.removed else fr.fts.index(q) for q in fr.key_pts]


def insert_one(cam, st, inp, b, dims, mutant=None):
    """one acting sequence: the arrays of `st` are rewritten in place; -> (status, new slot, removed slot, promoted, deleted)"""
    K, F, P, R = dims
    o = SequenceObjects(cam, st, b, dims)
    waiting = []
    for fr in o.frames:
        fr.removed, fr.mutant, fr.waiting = False, mutant, waiting
    if any(not 0 <= s < K for s in o.kf_list):
        return 2, -1, -1, 0, 0
    keyframes = [o.frames[s] for s in o.kf_list]                       # Map::keyframes_
    free = [s for s in range(K) if s not in o.kf_list]
    n = min(max(int(inp["n"][b]), 0), inp["has_point"].shape[1])
    if not free or n > F:
        return 1, -1, -1, 0, 0
    new = o.frames[free[0]]
    was_keyframe = list(keyframes)

    # the frame as the tracker leaves it: fts_ in row order, one feature per point (a later row with the same point has none)
    new.fts, seen = [], set()
    for j in range(n):
        raw = int(inp["ftr_point"][b, j]) if inp["has_point"][b, j] else -1
        pt = o.points.get(raw) if raw not in seen else None
        if pt is not None:
            seen.add(raw)
        ftr = Feature(new, inp["px"][b, j].copy(), inp["f"][b, j].copy(), int(inp["level"][b, j]), pt, raw)
        ftr.written = True
        new.fts.append(ftr)
    new.n_fts_written = new.key_pts_written = True
    new.key_pts = [new.fts[int(r)] if 0 <= int(r) < n else None for r in inp["key_pts"][b]]      # setKeyframe(), done by K11

    def add_frame_refs():                                               # frame_handler_mono.cpp:197-199, point.cpp:60-64
        for row, ftr in enumerate(new.fts):
            if ftr.point is not None:
                if len(ftr.point.obs) + 1 > R:
                    raise Overflow
                rec = Record(new.g, row, ftr.level, ftr.px, ftr.f, new)
                if mutant == "push_back":
                    ftr.point.obs.append(rec)
                else:
                    ftr.point.obs.insert(0, rec)
                ftr.point.stored()

    promoted = [0]

    def add_candidates_to_frame():                                      # map.cpp:220-237
        candidates = sorted((pt for pt in o.points.values() if pt.type == CANDIDATE), key=lambda pt: (pt.order, pt.index))
        for pt in candidates:
            if pt.obs and pt.obs[0].frame is new:
                own = pt.obs[-1]                                        # PointCandidate::second, the Feature the seed was made of
                if len(pt.obs) < 2 or own.row != -1 or own.frame is None or own.frame not in was_keyframe:
                    continue
                pt.type = UNKNOWN
                ftr = Feature(own.frame, own.px, own.f, own.level, None, -1)
                ftr.set_point(pt)
                own.frame.addFeature(ftr, F)
                own.row = len(own.frame.fts) - 1
                pt.stored()
                promoted[0] += 1

    deleted = [0]

    def safe_delete_frame(frame):                                       # map.cpp:41-64
        walk = frame.fts[:frame.n_before] if mutant == "appended_skipped" else list(frame.fts)
        seen = set()
        for ftr in walk:                                                # removePtFrameRef, map.cpp:66-80
            pt = ftr.point
            if pt is None or pt.index in seen or pt.type == DELETED:
                continue
            seen.add(pt.index)
            ftr.set_point(None)
            if len(pt.obs) <= (1 if mutant == "delete_at_one" else 2):
                for rec in pt.obs:                                      # safeDeletePoint, map.cpp:82-93
                    if rec.feature() is not None and rec.frame is not frame:
                        rec.feature().set_point(None)
                        rec.frame.removeKeyPoint(rec.feature())
                pt.obs = []
                pt.type = DELETED                                       # deletePoint
                deleted[0] += 1
                continue
            for i, rec in enumerate(pt.obs):                            # Point::deleteFrameRef, point.cpp:74-85
                if rec.kf == frame.g:
                    del pt.obs[i]
                    pt.stored()
                    break
        for fr in waiting:
            fr.setKeyPoints()
        keyframes.remove(frame)
        for ftr in frame.fts:
            ftr.set_point(None)
        frame.removed = frame.n_fts_written = frame.key_pts_written = True
        for pt in o.points.values():                                    # removeFrameCandidates, map.cpp:254-268
            if pt.type == CANDIDATE and pt.obs and pt.obs[-1].row == -1 and pt.obs[-1].kf == frame.g:
                pt.type, pt.obs = DELETED, []
                deleted[0] += 1

    rm = int(inp["kf_remove"][b])
    furthest = keyframes[rm] if 0 <= rm < len(keyframes) else None
    for fr in o.frames:
        fr.n_before = len(fr.fts)
    try:
        steps = [add_frame_refs, add_candidates_to_frame]
        if mutant == "promote_before_frame_ref":
            steps.reverse()
        if mutant == "remove_before_promote" and furthest is not None:
            add_frame_refs()
            safe_delete_frame(furthest)
            add_candidates_to_frame()
        else:
            for step in steps:
                step()
            if furthest is not None:                                    # frame_handler_mono.cpp:224-229
                safe_delete_frame(furthest)
    except Overflow:
        return 1, -1, -1, 0, 0
    if mutant == "new_frame_at_front":
        keyframes.insert(0, new)
    else:
        keyframes.append(new)                                           # Map::addKeyframe
    o.write_back(st)
    g = new.g
    st["kf_T"][g], st["kf_store_slot"][g] = inp["T_out"][b], inp["slot"][b]
    st["kf_list"][b] = [fr.slot for fr in keyframes] + [-1] * (K - len(keyframes))
    st["n_kf"][b] = len(keyframes)
    return 0, new.slot, -1 if furthest is None else furthest.slot, promoted[0], deleted[0]


def insert(cam, state, inp, mutant=None):
    """-> (the state after the call, the outputs): svo_hip_keyframe_insert on copies of the arrays"""
    B, K = state["kf_list"].shape
    F, P, R = state["ftr_point"].shape[1], state["pt_type"].shape[1], state["obs_kf"].shape[2]
    out = {k: np.zeros(B, np.int32) for k in OUTPUTS}
    out["kf_new_slot"][:] = -1
    out["kf_removed_slot"][:] = -1
    st = {k: np.array(state[k], copy=True) for k in STATE}
    for b in range(B):
        if int(inp["result"][b]) != RESULT_IS_KEYFRAME:
            continue
        trial = {k: v.copy() for k, v in st.items()}                    # (a sequence that overflows leaves its state as it was)
        res = insert_one(cam, trial, inp, b, (K, F, P, R), mutant)
        if res[0] == 0:
            st = trial
        for k, v in zip(OUTPUTS, res):
            out[k][b] = v
    return st, out
