"""Batched host mirrors of the reference classes that run after sparse alignment, over the
C ABI (include/svo_hip.h).  Names and argument meaning follow the reference:

  feature_alignment.align2D / align1D   svo/include/svo/feature_alignment.h:29-44
  Matcher.findMatchDirect               svo/include/svo/matcher.h:106-111
  Reprojector.reprojectPoint            svo/src/reprojector.cpp:206-217
  pose_optimizer.optimizeGaussNewton    svo/include/svo/pose_optimizer.h:37-45
  Point.optimize                        svo/include/svo/point.h:85
  DepthFilter.updateSeeds / updateSeed  svo/include/svo/depth_filter.h:120-135,158

Every call takes device-resident torch tensors (torch is the allocator / stream provider
only) and enqueues on the current stream.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import capi
from .pyramid import PyramidStore, _stream_ptr


def _ptr(t):
    return None if t is None else t.data_ptr()


def _chk(t, dtype):
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous(), "device-resident contiguous tensor required"
    return t


class FrameTable:
    """Device mirror of the svo::Frame objects a batch refers to: pyramid slot + T_f_w_."""

    def __init__(self, slot: torch.Tensor, T_f_w: torch.Tensor):
        self.slot = _chk(slot, torch.int32)
        self.T_f_w = _chk(T_f_w, torch.float64)
        assert T_f_w.shape == (slot.shape[0], 12)

    def struct(self) -> capi.Frames:
        return capi.Frames(self.slot.shape[0], 0, self.slot.data_ptr(), self.T_f_w.data_ptr())


@dataclass
class FeatureSet:
    """SoA of svo::Feature (feature.h:26-71)."""
    frame: torch.Tensor            # [n] i32 index into a FrameTable
    level: torch.Tensor            # [n] i32
    px: torch.Tensor               # [n,2] f64
    f: torch.Tensor                # [n,3] f64
    type: torch.Tensor | None = None   # [n] u8
    grad: torch.Tensor | None = None   # [n,2] f64

    def struct(self) -> capi.Features:
        _chk(self.frame, torch.int32); _chk(self.level, torch.int32); _chk(self.px, torch.float64); _chk(self.f, torch.float64)
        if self.type is not None:
            _chk(self.type, torch.uint8); _chk(self.grad, torch.float64)
        return capi.Features(self.frame.data_ptr(), self.level.data_ptr(), _ptr(self.type), self.px.data_ptr(),
                             self.f.data_ptr(), _ptr(self.grad))


class _Workspace:
    def __init__(self):
        self.buf = None

    def get(self, lib, M: int, device):
        need = lib.svo_hip_match_workspace_bytes(M)
        if self.buf is None or self.buf.numel() < need or self.buf.device != device:
            self.buf = torch.empty(need, dtype=torch.uint8, device=device)
        return self.buf


# ---- feature_alignment ----------------------------------------------------------------
def align_batch(store: PyramidStore, slot, level, patch_with_border, px, n_iter: int, dir=None, use_1d=None, phased: bool = False,
                evaluations=None):
    """feature_alignment::align2D (use_1d None/0) or align1D per trial.  px [M,2] f64 is refined
    in place (level coordinates).  Returns (ok [M] i32, h_inv [M] f64).  phased: run the iterations in three
    launches with the unfinished trials compacted in between (svo_hip_align_batch_phased; same results)."""
    lib = capi.load()
    M = px.shape[0]
    if phased:
        _chk(slot, torch.int32); _chk(level, torch.int32); _chk(patch_with_border, torch.uint8); _chk(px, torch.float64)
        ok = torch.zeros(M, dtype=torch.int32, device=px.device)
        h_inv = torch.zeros(M, dtype=torch.float64, device=px.device)
        ws = torch.empty(max(int(lib.svo_hip_align_workspace_bytes(M)), 256), dtype=torch.uint8, device=px.device)
        capi.check(lib.svo_hip_align_batch_phased(C.byref(store.layout), store.ptr, M, slot.data_ptr(), level.data_ptr(),
                                                  patch_with_border.data_ptr(), _ptr(dir), _ptr(use_1d), n_iter, px.data_ptr(),
                                                  ok.data_ptr(), h_inv.data_ptr(), _ptr(evaluations), ws.data_ptr(), ws.numel(),
                                                  _stream_ptr(store.device)), "svo_hip_align_batch_phased")
        return ok, h_inv
    _chk(slot, torch.int32); _chk(level, torch.int32); _chk(patch_with_border, torch.uint8); _chk(px, torch.float64)
    assert patch_with_border.shape == (M, 100)
    ok = torch.zeros(M, dtype=torch.int32, device=px.device)
    h_inv = torch.zeros(M, dtype=torch.float64, device=px.device)
    capi.check(lib.svo_hip_align_batch(C.byref(store.layout), store.ptr, M, slot.data_ptr(), level.data_ptr(),
                                       patch_with_border.data_ptr(), _ptr(dir), _ptr(use_1d), n_iter, px.data_ptr(),
                                       ok.data_ptr(), h_inv.data_ptr(), _stream_ptr(store.device)), "svo_hip_align_batch")
    return ok, h_inv


# ---- Matcher ----------------------------------------------------------------------------
@dataclass
class MatchResult:
    ok: torch.Tensor            # [M] i32   findMatchDirect's return value
    px_cur: torch.Tensor        # [M,2] f64 refined pixel (level 0)
    ref_obs: torch.Tensor       # [M] i32   observation chosen as ref_ftr_
    search_level: torch.Tensor  # [M] i32
    A_cur_ref: torch.Tensor     # [M,4] f64
    patch_with_border: torch.Tensor  # [M,100] u8


class Matcher:
    """Batched svo::Matcher (matcher.h:64-127): options as in Matcher::Options."""

    def __init__(self, align_max_iter: int = 10, n_pyr_levels: int = 3):
        self.align_max_iter = align_max_iter
        self.n_pyr_levels = n_pyr_levels  # Config::nPyrLevels()
        self.lib = capi.load()
        self._ws = _Workspace()

    def alloc_result(self, M: int, device) -> MatchResult:
        return MatchResult(torch.zeros(M, dtype=torch.int32, device=device), torch.zeros(M, 2, dtype=torch.float64, device=device),
                           torch.zeros(M, dtype=torch.int32, device=device), torch.zeros(M, dtype=torch.int32, device=device),
                           torch.zeros(M, 4, dtype=torch.float64, device=device),
                           torch.zeros(M, 100, dtype=torch.uint8, device=device))

    def find_match_direct(self, store: PyramidStore, cam, frames: FrameTable, cur_frame, pt_pos, obs_ptr,
                          obs: FeatureSet, px_cur, out: MatchResult | None = None) -> MatchResult:
        """out: a result block from alloc_result() to reuse (every field is overwritten by the
        kernels; px_cur is copied into out.px_cur first)."""
        M = pt_pos.shape[0]
        dev = store.device
        _chk(cur_frame, torch.int32); _chk(pt_pos, torch.float64); _chk(obs_ptr, torch.int32); _chk(px_cur, torch.float64)
        res = out if out is not None else self.alloc_result(M, dev)
        res.px_cur.copy_(px_cur)
        ws = self._ws.get(self.lib, M, dev)
        c, fr, ob = capi.camera(cam), frames.struct(), obs.struct()
        capi.check(self.lib.svo_hip_find_match_direct(
            C.byref(store.layout), store.ptr, C.byref(c), C.byref(fr), M, cur_frame.data_ptr(), pt_pos.data_ptr(),
            obs_ptr.data_ptr(), C.byref(ob), self.n_pyr_levels, self.align_max_iter, res.px_cur.data_ptr(),
            res.ok.data_ptr(), res.ref_obs.data_ptr(), res.search_level.data_ptr(), res.A_cur_ref.data_ptr(),
            res.patch_with_border.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(dev)), "svo_hip_find_match_direct")
        return res


def find_epipolar_match_direct(store: PyramidStore, cam, frames: FrameTable, cur_frame, ftr: FeatureSet, d_estimate, d_min,
                               d_max, n_pyr_levels: int = 3, align_1d: bool = False, align_max_iter: int = 10,
                               max_epi_search_steps: int = 1000, subpix_refinement: bool = True,
                               epi_search_edgelet_filtering: bool = True, epi_search_edgelet_max_angle: float = 0.7):
    """Batched Matcher::findEpipolarMatchDirect (matcher.h:113-123) for S queries.  Returns
    (ok [S] i32, depth [S] f64, px_cur [S,2], search_level [S] i32)."""
    lib = capi.load()
    S = ftr.px.shape[0]
    dev = store.device
    opt = capi.DepthFilterOptions(0, 0, 0.0, int(align_1d), align_max_iter, max_epi_search_steps, int(subpix_refinement),
                                  int(epi_search_edgelet_filtering), n_pyr_levels, epi_search_edgelet_max_angle)
    ok = torch.zeros(S, dtype=torch.int32, device=dev)
    depth = torch.zeros(S, dtype=torch.float64, device=dev)
    px = torch.zeros(S, 2, dtype=torch.float64, device=dev)
    lvl = torch.zeros(S, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.svo_hip_match_workspace_bytes(S), dtype=torch.uint8, device=dev)
    c, fr, ft = capi.camera(cam), frames.struct(), ftr.struct()
    capi.check(lib.svo_hip_find_epipolar_match_direct(
        C.byref(store.layout), store.ptr, C.byref(c), C.byref(fr), S, _chk(cur_frame, torch.int32).data_ptr(), C.byref(ft),
        _chk(d_estimate, torch.float64).data_ptr(), _chk(d_min, torch.float64).data_ptr(), _chk(d_max, torch.float64).data_ptr(),
        C.byref(opt), ok.data_ptr(), depth.data_ptr(), px.data_ptr(), lvl.data_ptr(), ws.data_ptr(), ws.numel(),
        _stream_ptr(dev)), "svo_hip_find_epipolar_match_direct")
    return ok, depth, px, lvl


def reproject_points(cam, frames: FrameTable, cur_frame, pt_pos, cell_size: int, grid_n_cols: int, out=None):
    """Reprojector::reprojectPoint for M points: (cell [M] i32 (-1 = not in frame), px [M,2]).
    out: (cell, px) tensors to reuse."""
    lib = capi.load()
    M = pt_pos.shape[0]
    dev = pt_pos.device
    if out is not None:
        cell, px = out
    else:
        cell = torch.zeros(M, dtype=torch.int32, device=dev)
        px = torch.zeros(M, 2, dtype=torch.float64, device=dev)
    c, fr = capi.camera(cam), frames.struct()
    capi.check(lib.svo_hip_reproject_points(C.byref(c), C.byref(fr), M, _chk(cur_frame, torch.int32).data_ptr(),
                                            _chk(pt_pos, torch.float64).data_ptr(), cell_size, grid_n_cols,
                                            cell.data_ptr(), px.data_ptr(), _stream_ptr(dev)), "svo_hip_reproject_points")
    return cell, px


def compose_poses(A, B, out=None, out_index=None):
    """out[idx[i]] = A[i] * B[i] (SE3 product), e.g. T_f_w(cur) = T_cur_from_ref * T_f_w(ref)."""
    lib = capi.load()
    n = A.shape[0]
    if out is None:
        out = torch.empty_like(A)
    capi.check(lib.svo_hip_compose_poses(n, _chk(A, torch.float64).data_ptr(), _chk(B, torch.float64).data_ptr(),
                                         _chk(out, torch.float64).data_ptr(), _ptr(out_index), _stream_ptr(A.device)),
               "svo_hip_compose_poses")
    return out


def cam2world(cam, px, out=None):
    """Unit bearings of pixels px [n,2] (vk::PinholeCamera::cam2world)."""
    lib = capi.load()
    n = px.shape[0]
    if out is None:
        out = torch.empty(n, 3, dtype=torch.float64, device=px.device)
    c = capi.camera(cam)
    capi.check(lib.svo_hip_cam2world(C.byref(c), n, _chk(px, torch.float64).data_ptr(), out.data_ptr(),
                                     _stream_ptr(px.device)), "svo_hip_cam2world")
    return out


def select_matches(cam, cell, ok, px, level, pos, max_fts):
    """Reprojector::reprojectMap's cell loop over the results of M trials given in visiting order
    (svo/src/reprojector.cpp:131-139, 150-200): per cell the first trial that matched, at most max_fts + 1 of them.
    Returns (n [1] int32, sel, f, level_out, pos_out, has_point), the arrays min(M, max_fts + 1) long: the
    observations of the selected trials in Frame::fts_ order, as svo_hip_pose_optimize reads them."""
    lib = capi.load()
    M = cell.shape[0]
    dev = px.device
    cap = max(1, min(M, max_fts + 1))
    n = torch.zeros(1, dtype=torch.int32, device=dev)
    sel = torch.full((cap,), -1, dtype=torch.int32, device=dev)
    f = torch.zeros(cap, 3, dtype=torch.float64, device=dev)
    level_out = torch.zeros(cap, dtype=torch.int32, device=dev)
    pos_out = torch.zeros(cap, 3, dtype=torch.float64, device=dev)
    has_point = torch.zeros(cap, dtype=torch.uint8, device=dev)
    c = capi.camera(cam)
    capi.check(lib.svo_hip_select_matches(C.byref(c), M, _chk(cell, torch.int32).data_ptr(), _chk(ok, torch.int32).data_ptr(),
                                          _chk(px, torch.float64).data_ptr(), _chk(level, torch.int32).data_ptr(),
                                          _chk(pos, torch.float64).data_ptr(), int(max_fts), n.data_ptr(), sel.data_ptr(),
                                          f.data_ptr(), level_out.data_ptr(), pos_out.data_ptr(), has_point.data_ptr(),
                                          None, 0, _stream_ptr(dev)), "svo_hip_select_matches")
    return n, sel, f, level_out, pos_out, has_point


# ---- pose_optimizer ---------------------------------------------------------------------
@dataclass
class PoseOptResult:
    T_f_w: torch.Tensor       # [B,12]
    Cov: torch.Tensor         # [B,36]
    stats: torch.Tensor       # [B,4] estimated_scale, error_init, error_final, num_obs
    ran: torch.Tensor         # [B] i32 capi.POSE_RAN_*
    has_point: torch.Tensor   # [B,ns] u8 after pruning


def optimize_gauss_newton(cam, n, f, level, pos, has_point, T_f_w, reproj_thresh: float = 2.0, n_iter: int = 10,
                          ordered: bool = False, out: PoseOptResult | None = None, deferred: bool = False) -> PoseOptResult:
    """pose_optimizer::optimizeGaussNewton for B frames (reproj_thresh = Config::poseOptimThresh(),
    n_iter = Config::poseOptimNumIter(), frame_handler_mono.cpp:163-165).  ordered=True runs the
    kernel that adds the normal equations in the reference's observation order (the checker)."""
    lib = capi.load()
    B, ns = f.shape[0], f.shape[1]
    dev = f.device
    _chk(n, torch.int32); _chk(f, torch.float64); _chk(level, torch.int32); _chk(pos, torch.float64)
    _chk(has_point, torch.uint8); _chk(T_f_w, torch.float64)
    c = capi.camera(cam)
    if out is not None and not (ordered or deferred):
        # reuse a result block: the kernel reads the pose and the flags where they are and writes the block (no copies)
        _chk(out.has_point, torch.uint8); _chk(out.T_f_w, torch.float64)
        assert out.has_point.numel() == has_point.numel() == B * ns and out.T_f_w.numel() == T_f_w.numel() == 12 * B
        capi.check(lib.svo_hip_pose_optimize_into(C.byref(c), B, n.data_ptr(), ns, f.data_ptr(), level.data_ptr(), pos.data_ptr(),
                                                  has_point.data_ptr(), T_f_w.data_ptr(), reproj_thresh, n_iter,
                                                  out.has_point.data_ptr(), out.T_f_w.data_ptr(), out.Cov.data_ptr(),
                                                  out.stats.data_ptr(), out.ran.data_ptr(), _stream_ptr(dev)),
                   "svo_hip_pose_optimize_into")
        return out
    if out is not None:  # the in-place entries on a reused result block: pose and flags are in/out for the kernel
        res = out
        res.T_f_w.copy_(T_f_w)
        res.has_point.copy_(has_point)
    else:
        res = PoseOptResult(T_f_w.clone(), torch.zeros(B, 36, dtype=torch.float64, device=dev),
                            torch.zeros(B, 4, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev),
                            has_point.clone())
    # deferred: svo_hip_pose_optimize_deferred -- frames the wave kernel hands over come back untouched with
    # ran == capi.POSE_RAN_ORDERED
    fn = lib.svo_hip_pose_optimize_ordered if ordered else (lib.svo_hip_pose_optimize_deferred if deferred else lib.svo_hip_pose_optimize)
    capi.check(fn(C.byref(c), B, n.data_ptr(), ns, f.data_ptr(), level.data_ptr(), pos.data_ptr(),
                  res.has_point.data_ptr(), reproj_thresh, n_iter, res.T_f_w.data_ptr(),
                  res.Cov.data_ptr(), res.stats.data_ptr(), res.ran.data_ptr(), _stream_ptr(dev)),
               "svo_hip_pose_optimize")
    return res


# ---- the end of FrameHandlerMono::processFrame ------------------------------------------------
@dataclass
class FrameClose:
    """The outputs of svo_hip_frame_close for B sequences (include/svo_hip.h states every one)."""
    gate: torch.Tensor        # [B] i32   0, or the failure gate that stopped the frame (1 .. 3)
    quality: torch.Tensor     # [B] i32   capi.TRACKING_*
    result: torch.Tensor      # [B] i32   capi.RESULT_*
    T_out: torch.Tensor       # [B,12]    new_frame_->T_f_w_ as processFrame leaves it
    nobs_out: torch.Tensor    # [B] i32   Frame::nObs(): the next frame's num_obs_last
    depth_mean: torch.Tensor  # [B] f64
    depth_min: torch.Tensor   # [B] f64
    kf_block: torch.Tensor    # [B] i32   the keyframe that made needNewKf false, -1: none
    valid: torch.Tensor       # [B,ns] u8 K1's `valid` with this frame as the reference
    xyz_ref: torch.Tensor     # [B,ns,3]  K1's `xyz_ref` likewise
    key_pts: torch.Tensor     # [B,5] i32 rows, -1 = NULL
    occupancy: torch.Tensor   # [B,cells] u8, FastDetector.detect's occupancy
    kf_remove: torch.Tensor   # [B] i32   the keyframe getFurthestKeyframe picks, -1: none is removed


_FRAME_CLOSE_DTYPES = dict(gate=torch.int32, quality=torch.int32, result=torch.int32, T_out=torch.float64, nobs_out=torch.int32,
                           depth_mean=torch.float64, depth_min=torch.float64, kf_block=torch.int32, valid=torch.uint8,
                           xyz_ref=torch.float64, key_pts=torch.int32, occupancy=torch.uint8, kf_remove=torch.int32)


def frame_close_outputs(B: int, n_stride: int, cells: int, device) -> FrameClose:
    """The tensors of svo_hip_frame_close_out.  Allocate once and hand them to every call that a HIP graph captures."""
    shape = dict(T_out=(B, 12), valid=(B, n_stride), xyz_ref=(B, n_stride, 3), key_pts=(B, 5), occupancy=(B, cells))
    return FrameClose(**{k: torch.zeros(shape.get(k, (B,)), dtype=dt, device=device) for k, dt in _FRAME_CLOSE_DTYPES.items()})


def frame_close_params(**fields) -> capi.FrameCloseParams:
    """svo_hip_frame_close_params: the reference's Config values, with the given fields replaced"""
    p = capi.FrameCloseParams()
    capi.check(capi.load().svo_hip_frame_close_params_default(C.byref(p)), "svo_hip_frame_close_params_default")
    for k, v in fields.items():
        assert k in dict(capi.FrameCloseParams._fields_) and k != "reserved", k
        setattr(p, k, v)
    return p


def close_frame(cam, n, px, f, pos, has_point, T_f_w, T_last, num_obs, num_obs_last, n_kf, kf_T, kf_overlap, cell_size: int,
                grid_n_cols: int, grid_n_rows: int, params: capi.FrameCloseParams | None = None,
                out: FrameClose | None = None) -> FrameClose:
    """The end of FrameHandlerMono::processFrame for B frames (svo_hip_frame_close): failure gates, tracking quality, scene
    depth, needNewKf, and for a new keyframe its key points, the detector's occupancy and the keyframe to drop; K1's
    xyz_ref / valid for the next frame.  n [B] i32, px [B,ns,2] / f [B,ns,3] / pos [B,ns,3] f64 and has_point [B,ns] u8 are
    the frame's features as select_matches and optimize_gauss_newton leave them; T_f_w / T_last [B,12]; num_obs /
    num_obs_last [B] i32; the map's keyframes n_kf [B] i32, kf_T [B,nk,12], kf_overlap [B,nk] i32 (-1: not in
    overlap_kfs_).  params: frame_close_params(...).  out: a FrameClose to reuse (every element is overwritten).
    Enqueued on the current stream, not synchronised."""
    B, ns = has_point.shape
    nk = kf_overlap.shape[1]
    i32, f64 = torch.int32, torch.float64
    for t, dt, shape in ((n, i32, (B,)), (px, f64, (B, ns, 2)), (f, f64, (B, ns, 3)), (pos, f64, (B, ns, 3)), (has_point, torch.uint8, (B, ns)),
                         (T_f_w, f64, (B, 12)), (T_last, f64, (B, 12)), (num_obs, i32, (B,)), (num_obs_last, i32, (B,)), (n_kf, i32, (B,)),
                         (kf_T, f64, (B, nk, 12)), (kf_overlap, i32, (B, nk))):
        assert _chk(t, dt) is t and tuple(t.shape) == shape, (tuple(t.shape), shape)
    dev = has_point.device
    cells = grid_n_cols * grid_n_rows
    out = frame_close_outputs(B, ns, cells, dev) if out is None else out
    for k, dt in _FRAME_CLOSE_DTYPES.items():
        t = getattr(out, k)
        assert t.dtype == dt and t.is_contiguous() and t.device == dev
    assert tuple(out.occupancy.shape) == (B, cells) and tuple(out.valid.shape) == (B, ns) and tuple(out.gate.shape) == (B,)
    p = params if params is not None else frame_close_params()
    i = capi.FrameCloseIn(*[_ptr(t) for t in (n, px, f, pos, has_point, T_f_w, T_last, num_obs, num_obs_last, n_kf, kf_T, kf_overlap)])
    o = capi.FrameCloseOut(*[_ptr(getattr(out, k)) for k in capi.FRAME_CLOSE_OUTPUTS])
    c = capi.camera(cam)
    capi.check(capi.load().svo_hip_frame_close(C.byref(c), B, ns, nk, C.byref(i), int(cell_size), int(grid_n_cols), int(grid_n_rows), cells,
                                               C.byref(p), C.byref(o), _stream_ptr(dev)), "svo_hip_frame_close")
    return out


@dataclass
class TrackedFrame:
    """What track_from_first_map leaves on the device for n sequences (m = the first map's stride, cap = min(m, max_fts + 1))."""
    align: object               # SparseAlignResult of K1 (T_cur_from_ref, n_tracked, ...)
    frames: FrameTable          # rows [0, n): first keyframes, [n, 2n): second keyframes, [2n, 3n): the tracked frames
    order: torch.Tensor         # [n,m] i64  trial t of a sequence is map rank order[t] (the reprojector's visiting order)
    n_trials: torch.Tensor      # [n] i32    Reprojector::n_trials_: the points inside the frame
    match: MatchResult          # [n*m] findMatchDirect per trial, trials beyond n_trials skipped (ok == 0)
    n_matches: torch.Tensor     # [n] i32    Reprojector::n_matches_ = the frame's features
    sel: torch.Tensor           # [n,cap] i32 the trial behind each feature, -1 beyond n_matches
    px: torch.Tensor            # [n,cap,2]  the new frame's Feature::px ..
    f: torch.Tensor             # [n,cap,3]  .. f
    level: torch.Tensor         # [n,cap] i32
    pos: torch.Tensor           # [n,cap,3]  the features' points
    pose: PoseOptResult         # optimizeGaussNewton: T_f_w, stats, has_point after pruning
    num_obs: torch.Tensor       # [n] i32    sfba_n_edges_final
    close: FrameClose


def track_from_first_map(store: PyramidStore, cam, fm, kf_slots, kf_T, next_slots, grid, detector_grid, num_obs_last=None,
                         params: capi.FrameCloseParams | None = None, max_fts: int = 120, sia=None, matcher: Matcher | None = None,
                         close_out: FrameClose | None = None) -> TrackedFrame:
    """The first FrameHandlerMono::processFrame after the bootstrap (frame_handler_mono.cpp:129-193), for the n sequences of a
    FirstMap `fm` (initialization.KltHomographyInit.first_map), enqueued on the current stream without a host read:
      1. SparseImgAlign.run, second keyframe -> next image, on fm.px[:, 1] / fm.xyz_ref / fm.n_points with an identity prior;
      2. compose_poses: the new frame's T_f_w into the frame table;
      3. reproject_points of the map points (ranks beyond n_points are no trials);
      4. Matcher.find_match_direct with two observation records per point, view 0 then view 1 (Point::obs_ after the two
         addFrameRef calls of initialization.cpp:78-97, which push to the front);
      5. select_matches per sequence; 6. optimize_gauss_newton; 7. close_frame.
    kf_slots = (slots of the first keyframes, of the second) [n] i32 each, kf_T = (T_ref_w, T_cur_w) [n,12] each, next_slots
    [n] i32.  grid: map_mirror.Grid, the reprojector's grid with its cell order; detector_grid = (cell_size, n_cols, n_rows) of
    the feature detector, for the occupancy.  num_obs_last [n] i32 defaults to fm.n_points (Frame::nObs() of the second
    keyframe, what processSecondFrame leaves in num_obs_last_).
    Every map point is TYPE_UNKNOWN and a cell's list sort is stable, so the visiting order is a stable sort of the in-frame
    points by the rank of their cell; that sort, the gathers and the record offsets are torch operations (plumbing).
    The map is the two keyframes of the first map: kf_overlap is 0 for both -- overlap_kfs_ holds every close keyframe
    (reprojector.cpp:75-80); Map::getCloseKeyframes' visibility test of the key points is not mirrored."""
    from .sparse_img_align import SparseImgAlign
    dev = store.device
    n, m = fm.pos.shape[0], fm.pos.shape[1]
    M = n * m
    i32, f64 = torch.int32, torch.float64
    T_ref_w, T_cur_w = kf_T
    sia = sia if sia is not None else SparseImgAlign(4, 2)
    matcher = matcher if matcher is not None else Matcher()
    # 1. K1
    prior = torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=f64, device=dev).repeat(n, 1)
    align = sia.run(store, cam, _chk(kf_slots[1], i32), _chk(next_slots, i32), fm.n_points, fm.px[:, 1].contiguous(), fm.xyz_ref, prior)
    # 2. the frame table and the new frame's pose
    frame_T = torch.cat([T_ref_w, T_cur_w, T_cur_w]).contiguous()
    frames = FrameTable(torch.cat([kf_slots[0], kf_slots[1], next_slots]).contiguous(), frame_T)
    cur_rows = torch.arange(2 * n, 3 * n, dtype=i32, device=dev)
    compose_poses(align.T_cur_from_ref, _chk(T_cur_w, f64), out=frame_T, out_index=cur_rows)
    # 3. Reprojector::reprojectPoint
    cur_frame = cur_rows.repeat_interleave(m).contiguous()
    cell, px_proj = reproject_points(cam, frames, cur_frame, fm.pos.reshape(M, 3), grid.cell_size, grid.n_cols)
    rank = torch.arange(m, device=dev)[None, :]
    in_frame = (cell.view(n, m) >= 0) & (rank < fm.n_points[:, None])
    # the visiting order: cells in grid_.cell_order, the points of a cell in map order
    key = torch.where(in_frame, grid.cell_rank.long()[cell.view(n, m).clamp(min=0).long()], grid.n_cols * grid.n_rows)
    order = torch.sort(key, dim=1, stable=True).indices
    take = lambda t: torch.gather(t, 1, order.view(n, m, *([1] * (t.dim() - 2))).expand(n, m, *t.shape[2:])).contiguous()
    t_in = take(in_frame)
    t_cell = torch.where(t_in, take(cell.view(n, m)), -1).to(i32).contiguous()
    t_pos, t_px = take(fm.pos), take(px_proj.view(n, m, 2))
    n_trials = t_in.sum(dim=1, dtype=i32)
    # 4. two observation records per trial, compacted: the records of a skipped trial go to two spare slots at the end
    ptr = torch.zeros(M + 1, dtype=i32, device=dev)
    ptr[1:] = torch.cumsum(2 * t_in.reshape(M).to(i32), 0)
    first = torch.where(t_in.reshape(M), ptr[:-1].long(), 2 * M)
    second = torch.where(t_in.reshape(M), ptr[:-1].long() + 1, 2 * M + 1)
    obs = FeatureSet(frame=torch.zeros(2 * M + 2, dtype=i32, device=dev), level=torch.zeros(2 * M + 2, dtype=i32, device=dev),
                     px=torch.zeros(2 * M + 2, 2, dtype=f64, device=dev), f=torch.zeros(2 * M + 2, 3, dtype=f64, device=dev))
    seq = torch.arange(n, dtype=i32, device=dev).repeat_interleave(m)
    for view, at in ((0, first), (1, second)):
        obs.frame.index_copy_(0, at, seq + view * n)
        obs.px.index_copy_(0, at, take(fm.px[:, view]).reshape(M, 2))
        obs.f.index_copy_(0, at, take(fm.f[:, view]).reshape(M, 3))
    match = matcher.find_match_direct(store, cam, frames, cur_frame, t_pos.reshape(M, 3), ptr, obs, t_px.reshape(M, 2))
    # 5. the cell loop of reprojectMap, sequence by sequence
    picked = [select_matches(cam, t_cell[b], match.ok.view(n, m)[b], match.px_cur.view(n, m, 2)[b], match.search_level.view(n, m)[b],
                             t_pos[b], max_fts) for b in range(n)]
    n_matches = torch.cat([p[0] for p in picked])
    sel, f, level, pos, has_point = (torch.stack([p[k] for p in picked]).contiguous() for k in range(1, 6))
    chosen = sel >= 0
    px = torch.gather(match.px_cur.view(n, m, 2), 1, sel.clamp(min=0).long()[..., None].expand(-1, -1, 2))
    px = torch.where(chosen[..., None], px, 0.0).contiguous()
    # 6. pose_optimizer::optimizeGaussNewton from the aligned pose
    pose = optimize_gauss_newton(cam, n_matches, f, level, pos, has_point, frame_T[2 * n:])
    num_obs = pose.stats[:, 3].to(i32)
    # 7. the end of the frame
    last = fm.n_points if num_obs_last is None else num_obs_last
    two = torch.full((n,), 2, dtype=i32, device=dev)
    close = close_frame(cam, n_matches, px, f, pos, pose.has_point, pose.T_f_w, T_cur_w, num_obs, _chk(last, i32), two,
                        torch.stack([T_ref_w, T_cur_w], dim=1).contiguous(), torch.zeros(n, 2, dtype=i32, device=dev), *detector_grid,
                        params=params, out=close_out)
    return TrackedFrame(align, frames, order, n_trials, match, n_matches, sel, px, f, level, pos, pose, num_obs, close)


# ---- Point::optimize ----------------------------------------------------------------------
def point_optimize(frames: FrameTable, obs_ptr, obs_frame, obs_f, pos, n_iter: int = 5):
    """Point::optimize(n_iter) for P points; returns the optimised positions [P,3]."""
    lib = capi.load()
    out = _chk(pos, torch.float64).clone()
    fr = frames.struct()
    capi.check(lib.svo_hip_point_optimize(C.byref(fr), pos.shape[0], _chk(obs_ptr, torch.int32).data_ptr(),
                                          _chk(obs_frame, torch.int32).data_ptr(), _chk(obs_f, torch.float64).data_ptr(),
                                          n_iter, out.data_ptr(), _stream_ptr(pos.device)), "svo_hip_point_optimize")
    return out


# ---- DepthFilter ----------------------------------------------------------------------------
@dataclass
class SeedSet:
    """SoA of svo::Seed (depth_filter.h:35-51); updated in place."""
    a: torch.Tensor
    b: torch.Tensor
    mu: torch.Tensor
    z_range: torch.Tensor
    sigma2: torch.Tensor
    batch_id: torch.Tensor

    def struct(self) -> capi.Seeds:
        for t in (self.a, self.b, self.mu, self.z_range, self.sigma2):
            _chk(t, torch.float32)
        _chk(self.batch_id, torch.int32)
        return capi.Seeds(self.a.data_ptr(), self.b.data_ptr(), self.mu.data_ptr(), self.z_range.data_ptr(),
                          self.sigma2.data_ptr(), self.batch_id.data_ptr())


class DepthFilter:
    """Batched svo::DepthFilter::updateSeeds.  Options: DepthFilter::Options + Matcher::Options."""

    def __init__(self, max_n_kfs: int = 3, seed_convergence_sigma2_thresh: float = 200.0, n_pyr_levels: int = 3,
                 align_1d: bool = False, align_max_iter: int = 10, max_epi_search_steps: int = 1000,
                 subpix_refinement: bool = True, epi_search_edgelet_filtering: bool = True,
                 epi_search_edgelet_max_angle: float = 0.7):
        self.opt = capi.DepthFilterOptions(max_n_kfs, 0, seed_convergence_sigma2_thresh, int(align_1d), align_max_iter,
                                           max_epi_search_steps, int(subpix_refinement),
                                           int(epi_search_edgelet_filtering), n_pyr_levels, epi_search_edgelet_max_angle)
        self.lib = capi.load()
        self._ws = _Workspace()

    def update_seeds(self, store: PyramidStore, cam, frames: FrameTable, cur_frame, ftr: FeatureSet, seeds: SeedSet,
                     batch_counter: int, out=None):
        """Returns (status [S] i32 capi.SEED_*, xyz_world [S,3], px_cur [S,2]); out: those three to reuse."""
        S = seeds.mu.shape[0]
        dev = store.device
        self.opt.batch_counter = batch_counter
        if out is not None:
            status, xyz, px = out
        else:
            status = torch.zeros(S, dtype=torch.int32, device=dev)
            xyz = torch.zeros(S, 3, dtype=torch.float64, device=dev)
            px = torch.zeros(S, 2, dtype=torch.float64, device=dev)
        ws = self._ws.get(self.lib, S, dev)
        self.last_workspace = ws
        c, fr, ft, sd = capi.camera(cam), frames.struct(), ftr.struct(), seeds.struct()
        capi.check(self.lib.svo_hip_update_seeds(C.byref(store.layout), store.ptr, C.byref(c), C.byref(fr), S,
                                                 _chk(cur_frame, torch.int32).data_ptr(), C.byref(ft), C.byref(sd),
                                                 C.byref(self.opt), status.data_ptr(), xyz.data_ptr(), px.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _stream_ptr(dev)), "svo_hip_update_seeds")
        return status, xyz, px

    def update_seeds_resident(self, store: PyramidStore, cam, frames: FrameTable, cur_frame: int, slot_of, store_ftr: FeatureSet,
                              store_seeds: SeedSet, batch_counter: int):
        """svo_hip_update_seeds_resident (row N2): the S seeds at slots `slot_of` [S] i32 of a resident store (store_ftr /
        store_seeds: columns indexed by slot, FeatureSet.frame holding frame-table indices), all updated with frame
        `cur_frame` of the table.  Returns (status [S], xyz_world [S,3], px_cur [S,2], state [4,S] = a, b, mu, sigma2)."""
        S = slot_of.shape[0]
        dev = store.device
        self.opt.batch_counter = batch_counter
        status = torch.zeros(S, dtype=torch.int32, device=dev)
        xyz = torch.zeros(S, 3, dtype=torch.float64, device=dev)
        px = torch.zeros(S, 2, dtype=torch.float64, device=dev)
        state = torch.zeros(4, S, dtype=torch.float32, device=dev)
        ws = self._ws.get(self.lib, S, dev)
        c, fr, ft, sd = capi.camera(cam), frames.struct(), store_ftr.struct(), store_seeds.struct()
        capi.check(self.lib.svo_hip_update_seeds_resident(
            C.byref(store.layout), store.ptr, C.byref(c), C.byref(fr), int(cur_frame), S, _chk(slot_of, torch.int32).data_ptr(),
            C.byref(ft), C.byref(sd), C.byref(self.opt), status.data_ptr(), xyz.data_ptr(), px.data_ptr(), state.data_ptr(),
            ws.data_ptr(), ws.numel(), _stream_ptr(dev)), "svo_hip_update_seeds_resident")
        return status, xyz, px, state

    @staticmethod
    def initialize_seeds(cam, corner_xy, corner_level, corner_score, detection_threshold: float, frame_index, depth_mean, depth_min,
                         batch_id: int, seed_stride: int | None = None, out=None):
        """DepthFilter::initializeSeeds after detect, for n keyframes (svo_hip_initialize_seeds): corner_xy [n, cells, 2] /
        corner_level [n, cells] i32 and corner_score [n, cells] f32 are FastDetector.detect's, frame_index [n] i32 goes into
        the new features' `frame`, depth_mean / depth_min [n] f64 are addKeyframe's arguments (the minimum already halved),
        batch_id is Seed::batch_counter after its increment.  Returns (FeatureSet, SeedSet, n_seeds [n] i32) with columns
        [n, seed_stride]: records 0 .. n_seeds - 1 of a row in cell order, zeros behind them.  out: that triple to reuse."""
        lib = capi.load()
        n, cells = corner_score.shape
        stride = cells if seed_stride is None else int(seed_stride)
        dev = corner_score.device
        _chk(corner_xy, torch.int32); _chk(corner_level, torch.int32); _chk(corner_score, torch.float32)
        _chk(frame_index, torch.int32); _chk(depth_mean, torch.float64); _chk(depth_min, torch.float64)
        assert tuple(corner_xy.shape) == (n, cells, 2) and tuple(corner_level.shape) == (n, cells)
        assert frame_index.shape == depth_mean.shape == depth_min.shape == (n,)
        if out is not None:
            ftr, seeds, n_seeds = out
            assert tuple(seeds.mu.shape) == (n, stride)
        else:
            z = lambda dt, *tail: torch.zeros(n, stride, *tail, dtype=dt, device=dev)
            ftr = FeatureSet(z(torch.int32), z(torch.int32), z(torch.float64, 2), z(torch.float64, 3), z(torch.uint8), z(torch.float64, 2))
            seeds = SeedSet(z(torch.float32), z(torch.float32), z(torch.float32), z(torch.float32), z(torch.float32), z(torch.int32))
            n_seeds = torch.zeros(n, dtype=torch.int32, device=dev)
        fs, ss = ftr.struct(), seeds.struct()
        o = capi.SeedInitOut(_chk(n_seeds, torch.int32).data_ptr(), fs.d_frame, fs.d_level, fs.d_type, fs.d_px, fs.d_f, fs.d_grad,
                             ss.d_a, ss.d_b, ss.d_mu, ss.d_z_range, ss.d_sigma2, ss.d_batch_id)
        c = capi.camera(cam)
        capi.check(lib.svo_hip_initialize_seeds(C.byref(c), n, cells, corner_xy.data_ptr(), corner_level.data_ptr(),
                                                corner_score.data_ptr(), float(detection_threshold), frame_index.data_ptr(),
                                                depth_mean.data_ptr(), depth_min.data_ptr(), int(batch_id), stride, C.byref(o),
                                                _stream_ptr(dev)), "svo_hip_initialize_seeds")
        return ftr, seeds, n_seeds

    @staticmethod
    def seed_store_patch(slots, src_ftr: FeatureSet, src_seeds: SeedSet, store_ftr: FeatureSet, store_seeds: SeedSet):
        """svo_hip_seed_store_patch: record i of src_* goes to slot slots[i] of the store's columns."""
        lib = capi.load()
        p = capi.SeedPatch(int(slots.shape[0]), 0, _chk(slots, torch.int32).data_ptr(), src_ftr.struct(), src_seeds.struct())
        ft, sd = store_ftr.struct(), store_seeds.struct()
        capi.check(lib.svo_hip_seed_store_patch(C.byref(p), C.byref(ft), C.byref(sd), _stream_ptr(slots.device)), "svo_hip_seed_store_patch")

    @staticmethod
    def update_seed(x, tau2, seeds: SeedSet):
        """static DepthFilter::updateSeed(x, tau2, seed) for S independent measurements."""
        lib = capi.load()
        sd = seeds.struct()
        capi.check(lib.svo_hip_update_seed_batch(x.shape[0], _chk(x, torch.float32).data_ptr(),
                                                 _chk(tau2, torch.float32).data_ptr(), C.byref(sd),
                                                 _stream_ptr(x.device)), "svo_hip_update_seed_batch")
