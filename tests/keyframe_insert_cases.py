"""TEST INFRASTRUCTURE (numpy only): the cases of svo_hip_keyframe_insert (K12), one set for the emulated program, the sanitizer
program, the GPU and the reference harness.  A case is a batch of B <= 8 sequences (K 3..12, F <= 300, P <= 600, R <= 12): the
arrays of svo_hip_seq_map, one or more calls' inputs, and the checker's answer after every call (`expect`).  Sequences are
built the way a map grows -- keyframes in list order, every feature with a point pushed to the front of that point's records --
either at random (`random_seq`) or by hand (`Builder`), and flattened with the checker's layout.

`well_formed` says that the reference's own map.cpp / point.cpp / frame.cpp can run the case (tests/test_keyframe_insert_checker.py);
the cases whose indices cannot index are pinned by the checker alone."""
import functools
import types

import numpy as np

import keyframe_insert_checker as chk
from first_map_cases import CAMERAS, bearing

IS_KF, NO_KF, FAILURE = 1, 0, 2


class Builder:
    """one sequence: keyframes in Map::keyframes_ order, points by index, candidates, then the new frame"""

    def __init__(self, cam, K, F, P, R, n_stride):
        self.cam, self.dims, self.n_stride = cam, (K, F, P, R), n_stride
        self.kfs, self.points, self.new = [], {}, None

    def point(self, p, type_=chk.UNKNOWN, order=0):
        self.points.setdefault(p, types.SimpleNamespace(type=type_, order=order, obs=[], pos=np.array([0.1 * p, -0.05 * p, 2.0 + 0.01 * p])))
        return self.points[p]

    def keyframe(self, slot, px, points, key_pts="scan", store_slot=None, link=True):
        """a keyframe with feature rows px [k][2] and their points (-1: none); link=False leaves the points' records alone"""
        px = np.asarray(px, np.float64).reshape(-1, 2)
        kf = types.SimpleNamespace(slot=slot, px=px, points=list(points), level=[(3 * r + slot) % 3 for r in range(len(px))],
                                   store_slot=100 + slot if store_slot is None else store_slot, key_pts=key_pts,
                                   T=np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0.01 * slot, -0.02 * slot, 0.03 * slot]))
        self.kfs.append(kf)
        if link:
            for row, p in enumerate(kf.points):
                if p >= 0:
                    self.point(p).obs.insert(0, (slot, row, kf.level[row], px[row]))
        return kf

    def candidate(self, p, slot, px, order):
        """a candidate point whose own Feature (in no list) lies in keyframe `slot`"""
        self.point(p, chk.CANDIDATE, order).obs.insert(0, (slot, -1, 1, np.asarray(px, np.float64)))

    def append_feature(self, kf, px, p):
        """what an earlier promotion leaves: a feature at the end of the table, its record at the back of the point's list"""
        kf.px = np.vstack([kf.px, np.asarray(px, np.float64)[None]])
        kf.points.append(p)
        kf.level.append(1)
        self.point(p).obs.append((kf.slot, len(kf.px) - 1, 1, kf.px[-1]))

    def frame(self, px, points, has_point=None, key_pts="scan", kf_remove=-1, result=IS_KF, n=None, slot=7):
        px = np.asarray(px, np.float64).reshape(-1, 2)
        hp = [1 if p >= 0 else 0 for p in points] if has_point is None else list(has_point)
        self.new = types.SimpleNamespace(px=px, points=list(points), has_point=hp, key_pts=key_pts, kf_remove=kf_remove, result=result,
                                         n=len(px) if n is None else n, slot=slot)
        return self

    def scan(self, px, has):
        """Frame::setKeyPoints on a frame that had none: rows"""
        fr = chk.Frame(self.cam, 0, 0)
        fr.fts = [chk.Feature(fr, q, None, 0, True if h else None, -1) for q, h in zip(px, has)]
        fr.setKeyPoints()
        return [-1 if q is None else fr.fts.index(q) for q in fr.key_pts]

    def write(self, b, st, inp):
        K, F, P, R = self.dims
        live = lambda p: p in self.points and self.points[p].type != chk.DELETED
        st["n_kf"][b] = len(self.kfs)
        for i, kf in enumerate(self.kfs):
            g = b * K + kf.slot
            st["kf_list"][b, i] = kf.slot
            k = len(kf.px)
            st["kf_store_slot"][g], st["kf_T"][g], st["kf_n_fts"][g] = kf.store_slot, kf.T, k
            st["ftr_px"][g, :k], st["ftr_f"][g, :k] = kf.px, bearing(self.cam, kf.px) if k else 0
            st["ftr_level"][g, :k], st["ftr_point"][g, :k] = kf.level, kf.points
            st["kf_key_pts"][g] = self.scan(kf.px, [live(p) for p in kf.points]) if isinstance(kf.key_pts, str) else kf.key_pts
        for p, pt in self.points.items():
            st["pt_pos"][b, p], st["pt_type"][b, p], st["pt_order"][b, p], st["pt_n_obs"][b, p] = pt.pos, pt.type, pt.order, len(pt.obs)
            for r, (slot, row, level, px) in enumerate(pt.obs):
                st["obs_kf"][b, p, r], st["obs_row"][b, p, r], st["obs_level"][b, p, r] = b * K + slot, row, level
                st["obs_px"][b, p, r], st["obs_f"][b, p, r] = px, bearing(self.cam, px[None])[0]
        self.write_frame(b, inp)

    def write_frame(self, b, inp):
        f, k = self.new, min(len(self.new.px), self.n_stride)
        live = lambda p: p in self.points and self.points[p].type != chk.DELETED
        inp["result"][b], inp["n"][b], inp["slot"][b], inp["kf_remove"][b] = f.result, f.n, f.slot, f.kf_remove
        inp["px"][b, :k], inp["f"][b, :k] = f.px[:k], bearing(self.cam, f.px[:k]) if k else 0
        inp["level"][b, :k], inp["has_point"][b, :k], inp["ftr_point"][b, :k] = [r % 3 for r in range(k)], f.has_point[:k], f.points[:k]
        inp["T_out"][b] = [1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, 0.25, -0.125]
        has = [h and live(p) for h, p in zip(f.has_point[:k], f.points[:k])]
        inp["key_pts"][b] = self.scan(f.px[:k], has) if isinstance(f.key_pts, str) else f.key_pts


def empty_inputs(B, n_stride):
    i, d = np.int32, np.float64
    z = lambda *s, dt=i: np.zeros(s, dt)
    inp = dict(result=z(B), n=z(B), px=z(B, n_stride, 2, dt=d), f=z(B, n_stride, 3, dt=d), level=z(B, n_stride), has_point=z(B, n_stride, dt=np.uint8),
               ftr_point=z(B, n_stride), T_out=z(B, 12, dt=d), slot=z(B), key_pts=z(B, 5), kf_remove=z(B))
    inp["ftr_point"][...] = -1
    inp["key_pts"][...] = -1
    inp["kf_remove"][...] = -1
    return inp


def random_px(rng, cam, k, whole):
    """k pixels inside the image: whole numbers (ties, the centre lines) or sixteenths"""
    px = np.stack([rng.integers(1, cam.width - 1, k), rng.integers(1, cam.height - 1, k)], axis=1).astype(np.float64)
    return px if whole else px + rng.integers(0, 16, (k, 2)) / 16.0


def random_seq(cam, dims, n_stride, seed, n_kf, per_kf, n_new, kf_remove, n_cand=6, whole=False, result=IS_KF, max_obs=4, slots=None, loose=8,
               n_pts=None, match_cands=0.6):
    """a well-formed map of n_kf keyframes, each point seen by 1 .. max_obs of them, n_cand candidates, and a frame of n_new rows:
    matches of points and of candidates, rows without a point, rows whose point was pruned"""
    K, F, P, R = dims
    rng = np.random.default_rng(seed)
    b = Builder(cam, K, F, P, R, n_stride)
    slots = list(rng.permutation(K)[:n_kf]) if slots is None else slots
    n_pts = max(1, (n_kf * per_kf) // 2) if n_pts is None else n_pts
    seen_by = [set(rng.choice(n_kf, size=min(n_kf, int(rng.integers(1, max_obs + 1))), replace=False)) if n_kf else set() for _ in range(n_pts)]
    for i in range(n_kf):
        mine = [p for p in range(n_pts) if i in seen_by[p]][:max(per_kf - loose, 0)]
        points = list(rng.permutation(mine + [-1] * min(loose, per_kf)))
        b.keyframe(int(slots[i]), random_px(rng, cam, len(points), whole), [int(p) for p in points])
    cands = list(range(n_pts, n_pts + (n_cand if n_kf else 0)))
    for c in cands:
        b.candidate(c, int(slots[int(rng.integers(0, n_kf))]), random_px(rng, cam, 1, whole)[0], int(rng.integers(0, 4)))
    known = [p for p in b.points if p < n_pts]
    pick = list(rng.permutation(known))[:max(n_new - 12, 0)] + [c for c in cands if rng.random() < match_cands]
    pick = [int(p) for p in pick][:n_new]
    points = list(rng.permutation(pick + [-1] * max(min(12, n_new), n_new - len(pick))))[:n_new]
    has = [0 if p < 0 or rng.random() < 0.1 else 1 for p in points]
    b.frame(random_px(rng, cam, len(points), whole), points, has_point=has, kf_remove=kf_remove, result=result, slot=int(rng.integers(0, 50)))
    return b


def batch(name, cam, dims, n_stride, builders, calls=1, well_formed=True, edit=None, later=None):
    """builders -> state and inputs.  edit(state, inp): what a hand-made case changes in the arrays.  later: builders of the
    frames of a second call (their keyframes are ignored)."""
    B = len(builders)
    st = chk.empty_state(B, *dims)
    inputs = [empty_inputs(B, n_stride)]
    for b, bd in enumerate(builders):
        bd.write(b, st, inputs[0])
    if later is not None:
        inputs.append(empty_inputs(B, n_stride))
        for b, bd in enumerate(later):
            bd.write_frame(b, inputs[1])
    if edit is not None:
        edit(st, inputs[0])
    expect, cur = [], st
    for inp in inputs:
        cur, out = chk.insert(cam, cur, inp)
        expect.append((cur, out))
    return types.SimpleNamespace(name=name, cam=cam, dims=dims, n_stride=n_stride, B=B, state=st, inputs=inputs, expect=expect, well_formed=well_formed)


HAND_DIMS = (5, 24, 40, 4)


def _hand(cam, dims=HAND_DIMS, n_stride=16):
    return Builder(cam, *dims, n_stride)


def key_point_cases(cam):
    """the hand-built maps around Frame::removeKeyPoint.  Keyframe A (slot 0) leaves; B (slot 1) and C (slot 2) stay."""
    cu, cv = cam.width // 2, cam.height // 2
    out = {}

    def two_keyframes(extra=None, trigger=True, b_key_pts="scan"):
        # B: row 0 at the centre (key point 0), rows 1 .. 4 one per quadrant, row 5 a second feature of quadrant 1
        bd = _hand(cam)
        b_px = [[cu, cv], [cu + 6, cv + 5], [cu + 6, cv - 5], [cv - 6, cv - 5], [cv - 6, cv + 5], [cu + 3, cv + 3]]
        a_points = [0, 10, 11, -1] if trigger else [10, 11, -1]
        bd.keyframe(0, [[5 + 2 * r, 4 + r] for r in range(len(a_points))], a_points)
        kf_b = bd.keyframe(1, b_px, [0, 1, 2, 3, 4, 5], key_pts=b_key_pts)
        bd.keyframe(2, [[cu - 2, cv + 1], [cu + 4, cv + 4], [3, 3]], [10, 11, 12])
        bd.keyframe(3, [[cu + 1, cv - 1], [8, 8]], [10, 12])
        if isinstance(b_key_pts, str):                    # B's key points as its own features left them: before anything is appended
            kf_b.key_pts = bd.scan(kf_b.px, [True] * len(b_px))
        if extra:
            extra(bd, kf_b)
        if bd.new is None:
            bd.frame([[cu + 1, cv + 1], [4, 4], [cu - 5, 6]], [1, -1, 3], kf_remove=0)
        return bd

    # point 0 has two records (A, B) and is B's centre key point: it goes with A, B re-scans
    out["kp_other_keyframe"] = [two_keyframes()]
    # an appended feature (an earlier promotion) beats B's standing key point 1 -- found only when something triggers a re-scan
    better = lambda bd, kf_b: bd.append_feature(kf_b, [cu + 9, cv + 9], 6)
    out["kp_appended_no_trigger"] = [two_keyframes(better, trigger=False)]
    out["kp_appended_trigger"] = [two_keyframes(better, trigger=True)]
    # the standing key point 1 (row 5) ties with row 6 ... and is not the first of its value: it stays (from NULL, row 1 side wins)
    def tie(bd, kf_b):
        bd.append_feature(kf_b, [cu + 5, cv + 6], 7)     # 5 * 6 == 6 * 5: the product of row 1
    out["kp_tie_keeps_incumbent"] = [two_keyframes(tie, b_key_pts=[0, 6, 2, 3, 4])]

    # a candidate of A matched by the new frame, where it is a key point: promoted into A, deleted with A, the NEW frame re-scans
    def into_removed(bd, kf_b):
        bd.candidate(20, 0, [9, 9], 1)
        bd.frame([[cu, cv], [cu + 2, cv + 2], [cu + 7, cv - 3], [cu - 9, cv - 2]], [20, 1, 2, 3], kf_remove=0)
    out["kp_new_frame"] = [two_keyframes(into_removed)]

    # a point whose two records lie in B and C while A's feature still names it: both frames lose a key point at once
    def two_frames(bd, kf_b):
        kf_a = bd.kfs[0]
        kf_a.points[3] = 13
        bd.point(13).obs = [(1, 0, 0, kf_b.px[0]), (2, 0, 0, bd.kfs[2].px[0])]
        kf_b.points[0] = 13
        bd.kfs[2].points[0] = 13
        bd.points[0].obs = [o for o in bd.points[0].obs if o[0] != 1]
        bd.points[10].obs = [o for o in bd.points[10].obs if o[0] != 2]
    out["kp_two_frames"] = [two_keyframes(two_frames)]

    # two deletions hit B one after the other: point 0 (B's centre) first, then point 5, which the first re-scan had made key
    # point 1 over a standing key point that ties with an earlier row -- the final state alone would have kept that one
    def one_after_the_other(bd, kf_b):
        kf_a = bd.kfs[0]
        kf_a.points[3] = 5
        kf_a.points[1], kf_a.points[2] = -1, -1
        for p in (10, 11):
            bd.points[p].obs = [o for o in bd.points[p].obs if o[0] != 0]
        bd.points[5].obs.append((0, 3, kf_a.level[3], kf_a.px[3]))
        kf_b.px[5] = [cu + 8, cv + 8]                     # the best of quadrant 1
        bd.points[5].obs[0] = (1, 5, kf_b.level[5], kf_b.px[5])
        bd.append_feature(kf_b, [cu + 5, cv + 6], 7)      # row 6 ties with row 1
    out["kp_one_after_the_other"] = [two_keyframes(one_after_the_other, b_key_pts=[0, 6, 2, 3, 4])]
    return out


def candidate_cases(cam):
    cu, cv = cam.width // 2, cam.height // 2

    def base(cands, frame_points, kf_remove=-1):
        bd = _hand(cam)
        bd.keyframe(0, [[5, 4], [7, 5], [9, 6]], [0, 1, -1])
        bd.keyframe(1, [[cu, cv], [cu + 6, cv + 5], [cu + 6, cv - 5]], [0, 1, 2])
        bd.keyframe(2, [[cu - 2, cv + 1], [cu + 4, cv + 4]], [2, 1])
        for p, slot, order in cands:
            bd.candidate(p, slot, [10 + p, 3 + p % 5], order)
        bd.frame([[cu + r, cv - r] for r in range(len(frame_points))], frame_points, kf_remove=kf_remove)
        return bd

    return {"candidates": [
        base([], [0, 1, -1]),                                                           # none
        base([(20, 1, 0), (21, 1, 1), (22, 2, 2), (23, 0, 3)], [0, 20, -1, 22]),        # some matched, some not
        base([(20, 1, 5), (21, 1, 3), (22, 1, 4)], [20, 21, 22, 1]),                    # one origin, reversed order
        base([(22, 1, 2), (20, 1, 2), (21, 1, 2)], [21, 22, 20]),                       # equal order: the smaller index first
        base([(20, 0, 0), (21, 0, 1), (22, 1, 2)], [21, 1], kf_remove=0),               # 20's keyframe leaves: removeFrameCandidates
        base([(20, 2, 0), (21, 2, 0)], [20, 21, 0, 2], kf_remove=2),                    # promoted into the keyframe that leaves
    ]}


OVERFLOW_DIMS = (4, 6, 30, 3)


def overflow_cases(cam):
    """every capacity, one off either side, a full sequence next to a healthy one"""
    dims = OVERFLOW_DIMS

    def seq(n_kf=2, n_obs_of_0=2, origin_rows=5, frame_rows=3, kf_remove=-1):
        bd = Builder(cam, *dims, 8)
        for i in range(n_kf):
            rows = origin_rows if i == 0 else 2
            bd.keyframe(i, [[4 + r, 3 + i] for r in range(rows)], [0 if r == 0 and i < n_obs_of_0 else (-1 if r else 9 + i) for r in range(rows)])
        bd.candidate(20, 0, [11, 9], 0)
        bd.frame([[6 + r, 7] for r in range(frame_rows)], ([0, 20] + [-1] * 6)[:frame_rows], kf_remove=kf_remove)
        return bd

    # no slot (also when a keyframe leaves: the slot is chosen first), R, F by a promotion, F by the frame itself
    return {"overflow": [seq(), seq(n_kf=4), seq(n_kf=4, kf_remove=1), seq(n_kf=3, n_obs_of_0=3), seq(origin_rows=6), seq(frame_rows=7), seq()],
            "overflow_fits": [seq(n_kf=3), seq(n_kf=3, n_obs_of_0=2), seq(origin_rows=5), seq(frame_rows=6), seq(origin_rows=6, frame_rows=1)]}


def bad_index_cases(cam):
    """indices that cannot index: each is treated as NULL"""
    dims, ns = (4, 24, 40, 4), 16
    cu, cv = cam.width // 2, cam.height // 2
    K, F, P, R = dims

    def seq(kf_remove=0, result=IS_KF):
        bd = Builder(cam, *dims, ns)
        bd.keyframe(0, [[5, 4], [7, 5], [9, 6], [11, 7]], [0, 1, 2, -1])
        bd.keyframe(1, [[cu, cv], [cu + 6, cv + 5], [cu + 6, cv - 5], [cv - 6, cv - 5]], [0, 1, 2, 3])
        bd.keyframe(2, [[cu - 2, cv + 1], [cu + 4, cv + 4]], [3, 1])
        bd.candidate(20, 1, [12, 9], 0)
        bd.candidate(21, 0, [13, 9], 1)
        bd.frame([[cu + r, cv - r] for r in range(8)], [0, 20, 21, 3, -1, 1, 2, 3], kf_remove=kf_remove, result=result)
        return bd

    def edit(st, inp):
        inp["ftr_point"][0, :4] = [-5, P, P + 100, 2**31 - 1]                  # sequence 0: rows whose point is out of range
        inp["ftr_point"][1, 0] = 30                                            # 1: a point of type 0
        inp["ftr_point"][1, 3] = inp["ftr_point"][1, 5]                        #    and a second row with the point of a later one
        st["obs_kf"][2, 0, 0] = -1                                             # 2: records whose keyframe ..
        st["obs_kf"][2, 1, 0] = 3 * K + 9
        st["obs_kf"][2, 2, 1] = 0                                              #    (another sequence's frame)
        st["obs_row"][3, 0, 0] = 4                                             # 3: .. or row is outside its table
        st["obs_row"][3, 2, 1] = -2
        st["obs_row"][3, 1, 0] = 2**30
        st["obs_kf"][3, 20, 0] = 3 * K + 3                                     #    a candidate whose Feature lies in a free slot
        st["ftr_point"][4 * K + 0, 1] = P + 3                                  # 4: table rows of the leaving keyframe
        st["ftr_point"][4 * K + 0, 2] = -7
        st["ftr_point"][4 * K + 0, 3] = 30                                     #    (type 0)
        st["ftr_point"][4 * K + 1, 2] = 30
        st["kf_key_pts"][4 * K + 1] = [0, 99, -3, 3, 3]                        #    key points that are no rows
        inp["key_pts"][4] = [0, 8, -2, 99, 1]
        st["kf_n_fts"][4 * K + 2] = F + 9                                      #    a count beyond its capacity
        st["pt_n_obs"][5, 2], st["pt_n_obs"][5, 3] = R + 9, -4                 # 5: record counts beyond R (no room: status 1) ..
        st["pt_n_obs"][6, 3] = -4                                              # 6: .. and below zero

    builders = [seq(), seq(), seq(), seq(), seq(), seq(kf_remove=2), seq(kf_remove=2)]
    cases = {"bad_indices": (builders, edit)}

    def edit_remove(st, inp):
        inp["kf_remove"][:] = [-2, 3, 99, -1, 2**31 - 1, -2**31]
    cases["bad_kf_remove"] = ([seq() for _ in range(6)], edit_remove)

    def edit_list(st, inp):
        st["kf_list"][0, 1] = K
        st["kf_list"][1, 0] = -1
        st["kf_list"][2, 2] = 2**30
    cases["bad_kf_list"] = ([seq() for _ in range(4)], edit_list)
    return dims, ns, cases


@functools.lru_cache(maxsize=None)
def batches():
    """name -> batch (built once per process; the tests never write the arrays)"""
    wide, tiny, tall = (CAMERAS[k][0] for k in ("160x120", "47x33", "33x47"))
    out = []
    dims, ns = (6, 40, 120, 6), 48
    out.append(batch("removal_none_first_middle_last", wide, dims, ns,
                     [random_seq(wide, dims, ns, 10 + i, 4, 24, 30, rm) for i, rm in enumerate((-1, 0, 1, 2, 3))]))
    # a freed slot is taken by the next insertion
    first = [random_seq(wide, dims, ns, 20 + i, 5, 20, 28, rm, slots=[0, 1, 2, 3, 4]) for i, rm in enumerate((2, 0, -1))]
    second = [random_seq(wide, dims, ns, 30 + i, 5, 20, 28, rm) for i, rm in enumerate((1, -1, 0))]
    out.append(batch("freed_slot_reused", wide, dims, ns, first, later=second))
    # points with one, two and three records when their keyframe leaves; whole pixels on the small cameras: ties, centre lines
    for key, cam in (("47x33", tiny), ("33x47", tall), ("160x120", wide)):
        out.append(batch(f"few_records_{key}", cam, dims, ns,
                         [random_seq(cam, dims, ns, 40 + i, 4, 30, 36, i % 4, whole=True, max_obs=3, loose=3) for i in range(8)]))
    for key, cam in (("160x120", wide), ("47x33", tiny), ("33x47", tall)):
        for name, builders in {**key_point_cases(cam), **candidate_cases(cam)}.items():
            out.append(batch(f"{name}_{key}", cam, HAND_DIMS, 16, builders, well_formed=True))
    # -0 and +0 products: features on the centre lines, left and right, above and below
    cu, cv = tiny.width // 2, tiny.height // 2
    zeros = _hand(tiny)
    zeros.keyframe(0, [[5, 4], [6, 4]], [0, 1])
    zeros.keyframe(1, [[cu, cv - 3], [cu + 4, cv], [cu, cv + 2], [cu - 5, cv], [cu + 4, cv - 4], [cu, cv]], [0, 1, 2, 3, 4, 5], key_pts=[0, 1, 0, 3, 2])
    zeros.keyframe(2, [[4, 4]], [5])
    zeros.frame([[cu + 1, cv]], [4], kf_remove=0)
    out.append(batch("zero_products", tiny, HAND_DIMS, 16, [zeros]))
    for name, builders in overflow_cases(wide).items():
        out.append(batch(name, wide, OVERFLOW_DIMS, 8, builders))
    # the three results in one batch, identical sequences at different positions
    mixed = [random_seq(wide, dims, ns, 50 + i % 2, 4, 20, 30, 1, result=r) for i, r in enumerate((IS_KF, NO_KF, IS_KF, FAILURE, NO_KF, IS_KF, IS_KF, FAILURE))]
    out.append(batch("results_and_positions", wide, dims, ns, mixed))
    # 255 / 256 / 257 rows, and n beyond n_stride
    big, nb = (3, 300, 600, 4), 257
    rows = [random_seq(wide, big, nb, 60 + i, 2, 200, k, 0, loose=30) for i, k in enumerate((255, 256, 257))]
    rows.append(random_seq(wide, big, nb, 63, 2, 200, 257, 1, loose=30))
    rows[3].new.n = 300
    out.append(batch("rows_255_256_257", wide, big, nb, rows))
    bdims, bns, bad = bad_index_cases(wide)
    for name, (builders, edit) in bad.items():
        out.append(batch(name, wide, bdims, bns, builders, well_formed=False, edit=edit))
    return {b.name: b for b in out}


NAMES = tuple(batches())


def limit_batches():
    """the shapes at the limits, for the sanitizer program: K = 64, R = 64, 257 and 1024 rows (built on demand: they are large)"""
    wide = CAMERAS["160x120"][0]
    d1, d2 = (64, 1024, 2048, 64), (5, 300, 600, 6)
    a = batch("limit_1024_rows", wide, d1, 1024, [random_seq(wide, d1, 1024, 70 + i, n_kf, 40, rows, rm, max_obs=n_kf, loose=10)
                                                   for i, (n_kf, rows, rm) in enumerate(((63, 1024, 5), (64, 900, 0), (40, 1500, 39)))])
    b = batch("limit_257_rows", wide, d2, 257, [random_seq(wide, d2, 257, 80 + i, 4, 250, 257, i, loose=20) for i in range(3)])
    return {x.name: x for x in (a, b)}
