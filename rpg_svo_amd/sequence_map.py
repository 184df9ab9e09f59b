"""The resident map of B sequences (svo_hip_seq_map, include/svo_hip.h) and the keyframe that enters it
(svo_hip_keyframe_insert, csrc/keyframe_insert.hip): what FrameHandlerMono::processFrame does to svo::Map after
setKeyframe() (frame_handler_mono.cpp:196-200, 224-232), in device memory that outlives a frame.

Torch is the allocator and the stream provider; the one kernel is HIP.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, fields

import torch

from . import capi
from .pyramid import _stream_ptr
from .tracking import FeatureSet, FrameTable

_I32, _F64 = torch.int32, torch.float64
# name -> (dtype, shape given B, K, F, P, R)
_LAYOUT = dict(
    n_kf=(_I32, lambda B, K, F, P, R: (B,)), kf_list=(_I32, lambda B, K, F, P, R: (B, K)),
    kf_store_slot=(_I32, lambda B, K, F, P, R: (B * K,)), kf_T=(_F64, lambda B, K, F, P, R: (B * K, 12)),
    kf_n_fts=(_I32, lambda B, K, F, P, R: (B * K,)), kf_key_pts=(_I32, lambda B, K, F, P, R: (B * K, 5)),
    ftr_px=(_F64, lambda B, K, F, P, R: (B * K, F, 2)), ftr_f=(_F64, lambda B, K, F, P, R: (B * K, F, 3)),
    ftr_level=(_I32, lambda B, K, F, P, R: (B * K, F)), ftr_point=(_I32, lambda B, K, F, P, R: (B * K, F)),
    pt_pos=(_F64, lambda B, K, F, P, R: (B, P, 3)), pt_type=(_I32, lambda B, K, F, P, R: (B, P)),
    pt_order=(_I32, lambda B, K, F, P, R: (B, P)), pt_n_obs=(_I32, lambda B, K, F, P, R: (B, P)),
    obs_kf=(_I32, lambda B, K, F, P, R: (B, P, R)), obs_row=(_I32, lambda B, K, F, P, R: (B, P, R)),
    obs_level=(_I32, lambda B, K, F, P, R: (B, P, R)), obs_px=(_F64, lambda B, K, F, P, R: (B, P, R, 2)),
    obs_f=(_F64, lambda B, K, F, P, R: (B, P, R, 3)))
assert tuple(_LAYOUT) == capi.SEQ_MAP_FIELDS


def seq_map_shapes(B: int, K: int, F: int, P: int, R: int) -> dict:
    """name -> (shape, torch dtype) of every array of svo_hip_seq_map"""
    return {k: (shape(B, K, F, P, R), dt) for k, (dt, shape) in _LAYOUT.items()}


@dataclass
class SequenceMap:
    """svo_hip_seq_map: B maps with K keyframe storage slots of F features, P points of R observation records each.
    include/svo_hip.h states every array.  `cam` (width, height: the centre Frame::checkKeyPoints measures from) is what
    insert_keyframe hands to the kernel."""
    B: int
    K: int
    F: int
    P: int
    R: int
    n_kf: torch.Tensor
    kf_list: torch.Tensor
    kf_store_slot: torch.Tensor
    kf_T: torch.Tensor
    kf_n_fts: torch.Tensor
    kf_key_pts: torch.Tensor
    ftr_px: torch.Tensor
    ftr_f: torch.Tensor
    ftr_level: torch.Tensor
    ftr_point: torch.Tensor
    pt_pos: torch.Tensor
    pt_type: torch.Tensor
    pt_order: torch.Tensor
    pt_n_obs: torch.Tensor
    obs_kf: torch.Tensor
    obs_row: torch.Tensor
    obs_level: torch.Tensor
    obs_px: torch.Tensor
    obs_f: torch.Tensor
    cam: object = None

    @staticmethod
    def allocate(B: int, K: int, F: int, P: int, R: int, device, cam=None) -> "SequenceMap":
        """An empty map: no keyframe, no point (type 0), every index -1."""
        assert 1 <= K <= capi.SEQ_MAP_MAX_KFS and 1 <= F <= capi.SEQ_MAP_MAX_FTS and 1 <= P <= capi.SEQ_MAP_MAX_PTS and 1 <= R <= capi.SEQ_MAP_MAX_OBS
        t = {k: torch.zeros(shape, dtype=dt, device=device) for k, (shape, dt) in seq_map_shapes(B, K, F, P, R).items()}
        for k in ("kf_list", "kf_key_pts", "ftr_point", "obs_row"):
            t[k].fill_(-1)
        return SequenceMap(B, K, F, P, R, cam=cam, **t)

    @staticmethod
    def from_first_map(fm, kf_slots, kf_T, K: int = 10, F: int | None = None, P: int | None = None, R: int = 12, cam=None,
                       front_view: int = 1) -> "SequenceMap":
        """The map after the bootstrap (initialization.cpp:78-97), from a FirstMap of n sequences with stride m: the first
        keyframe in storage slot 0 and the second in slot 1, both feature tables in rank order, rank r = point r of type 2
        with two records, view `front_view` at the front and the other view behind it; FirstMap.key_pts copied.
        front_view = 1 (the default) puts the second keyframe's feature first; the reference's processSecondFrame calls
        addFrameRef for the current frame's feature and then for the reference frame's (:91, :95), which leaves view 0 in
        front -- front_view = 0 gives exactly that list (tracking.track_from_first_map's own two records are in that order).
        The order only breaks ties of Point::getCloseViewObs.
        kf_slots = (pyramid slots of the first keyframes, of the second) [n] i32, kf_T = (T_ref_w, T_cur_w) [n,12].
        Torch operations on the device only: nothing is read back."""
        assert front_view in (0, 1)
        n, m = fm.pos.shape[0], fm.pos.shape[1]
        F = m if F is None else F
        P = m if P is None else P
        assert F >= m and P >= m and R >= 2 and K >= 2
        dev = fm.pos.device
        s = SequenceMap.allocate(n, K, F, P, R, dev, cam=cam)
        live = torch.arange(m, device=dev)[None, :] < fm.n_points[:, None]          # [n, m]
        rank = torch.arange(m, dtype=_I32, device=dev)[None, :].expand(n, m)
        s.n_kf.fill_(2)
        s.kf_list[:, 0] = 0
        s.kf_list[:, 1] = 1
        g = torch.arange(n, dtype=_I32, device=dev) * K                             # frame of slot 0 per sequence
        for view in (0, 1):
            tab = s.ftr_px.view(n, K, F, 2)[:, view]
            tab[:, :m] = fm.px[:, view]
            s.ftr_f.view(n, K, F, 3)[:, view, :m] = fm.f[:, view]
            s.ftr_point.view(n, K, F)[:, view, :m] = torch.where(live, rank, -1)
            s.kf_n_fts.view(n, K)[:, view] = fm.n_points
            s.kf_key_pts.view(n, K, 5)[:, view] = fm.key_pts[:, view]
            s.kf_store_slot.view(n, K)[:, view] = kf_slots[view]
            s.kf_T.view(n, K, 12)[:, view] = kf_T[view]
            rec = 0 if view == front_view else 1
            s.obs_kf[:, :m, rec] = (g + view)[:, None]
            s.obs_row[:, :m, rec] = rank
            s.obs_px[:, :m, rec] = fm.px[:, view]
            s.obs_f[:, :m, rec] = fm.f[:, view]
        s.pt_pos[:, :m] = fm.pos
        s.pt_type[:, :m] = torch.where(live, capi.POINT_UNKNOWN, capi.POINT_DELETED).to(_I32)
        s.pt_n_obs[:, :m] = torch.where(live, 2, 0).to(_I32)
        return s

    def tensors(self) -> dict:
        return {k: getattr(self, k) for k in capi.SEQ_MAP_FIELDS}

    def struct(self) -> capi.SeqMap:
        for k, (shape, dt) in seq_map_shapes(self.B, self.K, self.F, self.P, self.R).items():
            t = getattr(self, k)
            assert t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == tuple(shape), k
        return capi.SeqMap(self.K, self.F, self.P, self.R, *[getattr(self, k).data_ptr() for k in capi.SEQ_MAP_FIELDS])

    def frame_table(self) -> FrameTable:
        """The B * K storage slots as a frame table (no copy): obs_kf indexes it."""
        return FrameTable(self.kf_store_slot, self.kf_T)

    def records(self) -> FeatureSet:
        """Every observation record as svo_hip_features columns (no copy): record r of point p of sequence b is row
        (b * P + p) * R + r, so a point's records are find_match_direct's obs rows [that row, + pt_n_obs)."""
        n = self.B * self.P * self.R
        return FeatureSet(frame=self.obs_kf.view(n), level=self.obs_level.view(n), px=self.obs_px.view(n, 2), f=self.obs_f.view(n, 3))

    def copy_(self, other: "SequenceMap") -> "SequenceMap":
        for k in capi.SEQ_MAP_FIELDS:
            getattr(self, k).copy_(getattr(other, k))
        return self

    def clone(self) -> "SequenceMap":
        return SequenceMap(self.B, self.K, self.F, self.P, self.R, cam=self.cam, **{k: getattr(self, k).clone() for k in capi.SEQ_MAP_FIELDS})


@dataclass
class KeyframeInsert:
    """The outputs of svo_hip_keyframe_insert for B sequences."""
    status: torch.Tensor             # [B] i32 0 ok, 1 a capacity was exceeded, 2 kf_list cannot index (state untouched)
    kf_new_slot: torch.Tensor        # [B] i32 the storage slot the keyframe took, -1: none
    kf_removed_slot: torch.Tensor    # [B] i32 the storage slot that was freed, -1: none (drop its seeds with a mask)
    n_promoted: torch.Tensor         # [B] i32 candidates that became points of the map
    n_points_deleted: torch.Tensor   # [B] i32


def keyframe_insert_outputs(B: int, device) -> KeyframeInsert:
    """Allocate once and hand to every call that a HIP graph captures."""
    return KeyframeInsert(*[torch.zeros(B, dtype=_I32, device=device) for _ in capi.KEYFRAME_INSERT_OUTPUTS])


def tracked_fields(tracked) -> dict:
    """The inputs of svo_hip_keyframe_insert from a tracking.TrackedFrame (torch on the device, no host read): the point
    behind a feature is the map rank of its trial, order[sel]."""
    n = tracked.sel.shape[0]
    chosen = tracked.sel >= 0
    rank = torch.gather(tracked.order, 1, tracked.sel.clamp(min=0).long())
    return dict(result=tracked.close.result, n=tracked.n_matches, px=tracked.px, f=tracked.f, level=tracked.level,
                has_point=tracked.pose.has_point, ftr_point=torch.where(chosen, rank, -1).to(_I32).contiguous(), T_out=tracked.close.T_out,
                slot=tracked.frames.slot[2 * n:3 * n].contiguous(), key_pts=tracked.close.key_pts, kf_remove=tracked.close.kf_remove)


def find_match_in_place(matcher, store, cam, smap: SequenceMap, cur_frame, point, n_trials, px_cur, out=None):
    """Matcher::findMatchDirect (svo_hip_find_match_direct_indirect) for trials whose observation records are read where
    they lie in `smap`: trial t < n_trials[0] is point `point[t]` (the flat index b * P + p, i64 or i32 [M]) seen from frame
    cur_frame[t] of smap.frame_table() -- a keyframe's slot, or a free slot the caller has given the frame's pyramid slot
    and pose.  n_trials [1] i32 stays on the device.  px_cur [M,2]: the projections.  Only the positions are gathered
    (plumbing); no record is copied.  -> tracking.MatchResult (out: one to reuse)."""
    M = point.shape[0]
    dev = smap.n_kf.device
    idx = point.long()
    begin = (idx * smap.R).to(_I32).contiguous()
    end = (begin + smap.pt_n_obs.view(-1)[idx].clamp(0, smap.R)).contiguous()
    pos = smap.pt_pos.view(-1, 3)[idx].contiguous()
    res = out if out is not None else matcher.alloc_result(M, dev)
    res.px_cur.copy_(px_cur)
    ws = matcher._ws.get(matcher.lib, M, dev)
    c, fr, ob = capi.camera(cam), smap.frame_table().struct(), smap.records().struct()
    assert cur_frame.dtype == _I32 and cur_frame.is_contiguous() and n_trials.dtype == _I32
    capi.check(matcher.lib.svo_hip_find_match_direct_indirect(
        C.byref(store.layout), store.ptr, C.byref(c), C.byref(fr), M, n_trials.data_ptr(), cur_frame.data_ptr(), pos.data_ptr(),
        begin.data_ptr(), end.data_ptr(), C.byref(ob), matcher.n_pyr_levels, matcher.align_max_iter, res.px_cur.data_ptr(),
        res.ok.data_ptr(), res.ref_obs.data_ptr(), res.search_level.data_ptr(), res.A_cur_ref.data_ptr(),
        res.patch_with_border.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(dev)), "svo_hip_find_match_direct_indirect")
    return res


def insert_keyframe(smap: SequenceMap, tracked_or_fields, out: KeyframeInsert | None = None, cam=None) -> KeyframeInsert:
    """svo_hip_keyframe_insert on `smap`, in place: for every sequence whose result is RESULT_IS_KEYFRAME the new frame's
    features become the front records of their points, matched candidates are promoted into their origin keyframes, the
    keyframe close_frame named is removed (points with two records or fewer deleted, key points repaired) and the new frame
    goes to the back of kf_list.  tracked_or_fields: a tracking.TrackedFrame, or a dict with capi.KEYFRAME_INSERT_INPUTS'
    names (result, n [B] i32; px [B,ns,2], f [B,ns,3] f64; level, ftr_point [B,ns] i32; has_point [B,ns] u8; T_out [B,12];
    slot [B] i32; key_pts [B,5] i32; kf_remove [B] i32).  out: a KeyframeInsert to reuse (every element is overwritten).
    Enqueued on the current stream, not synchronised."""
    fld = tracked_or_fields if isinstance(tracked_or_fields, dict) else tracked_fields(tracked_or_fields)
    cam = cam if cam is not None else smap.cam
    assert cam is not None, "the camera (width, height) is needed: SequenceMap.cam or cam="
    B = smap.B
    ns = fld["has_point"].shape[1]
    dts = dict(px=_F64, f=_F64, T_out=_F64, has_point=torch.uint8)
    shapes = dict(px=(B, ns, 2), f=(B, ns, 3), level=(B, ns), has_point=(B, ns), ftr_point=(B, ns), T_out=(B, 12), key_pts=(B, 5))
    dev = smap.n_kf.device
    for k in capi.KEYFRAME_INSERT_INPUTS:
        t = fld[k]
        assert t.is_cuda and t.device == dev and t.dtype == dts.get(k, _I32) and t.is_contiguous() and tuple(t.shape) == shapes.get(k, (B,)), k
    out = keyframe_insert_outputs(B, dev) if out is None else out
    for f_ in fields(out):
        t = getattr(out, f_.name)
        assert t.dtype == _I32 and t.is_contiguous() and t.device == dev and tuple(t.shape) == (B,), f_.name
    m = smap.struct()
    i = capi.KeyframeInsertIn(*[fld[k].data_ptr() for k in capi.KEYFRAME_INSERT_INPUTS])
    o = capi.KeyframeInsertOut(*[getattr(out, k).data_ptr() for k in capi.KEYFRAME_INSERT_OUTPUTS])
    c = capi.camera(cam)
    capi.check(capi.load().svo_hip_keyframe_insert(C.byref(c), B, ns, C.byref(m), C.byref(i), C.byref(o), _stream_ptr(dev)),
               "svo_hip_keyframe_insert")
    return out
