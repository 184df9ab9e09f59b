"""Batched host mirror of svo::initialization::KltHomographyInit (svo/src/initialization.cpp) over svo_hip_fast_detect,
svo_hip_cam2world, svo_hip_klt_track, svo_hip_klt_summarize (K8) and svo_hip_homography_init (K9).  Device-resident
tensors only; n independent sequences bootstrap side by side.

KltTracker is the tracking half (:29-54, 107-169): `add_frame` reports TRACKED for a sequence that has passed both gates
of addSecondFrame, and f_ref / f_cur / status / disparities are what computeHomography (:56) is given.
KltHomographyInit adds the rest (:56-98, 171-195): the robust homography, its decomposition, computeInliers, the
initMinInliers decision, the scale fix and the first map points, as include/svo_hip.h states them.
"""
from __future__ import annotations

import ctypes as C
import enum
from dataclasses import dataclass

import torch

from . import capi
from .feature_detection import FastDetector
from .pyramid import PyramidStore, _stream_ptr
from .tracking import DepthFilter, FeatureSet, SeedSet, cam2world


class InitResult(enum.IntEnum):
    """initialization.h's InitResult, plus TRACKED: both gates of addSecondFrame passed, the homography step is next."""
    FAILURE = 0
    NO_KEYFRAME = 1
    SUCCESS = 2
    TRACKED = 3


def klt_params() -> capi.KltParams:
    p = capi.KltParams()
    capi.check(capi.load().svo_hip_klt_params_default(C.byref(p)), "svo_hip_klt_params_default")
    return p


def klt_track(store: PyramidStore, ref_slot, cur_slot, px_ref, px_cur, status, error=None, params=None):
    """svo_hip_klt_track on tensors: ref_slot / cur_slot [n] i32, px_ref [n, m, 2] f32, px_cur (in: initial flow, out)
    and status [n, m] u8 are updated in place.  Returns error [n, m] f32."""
    n, m = px_ref.shape[:2]
    dev = store.device
    for t, dt in ((ref_slot, torch.int32), (cur_slot, torch.int32), (px_ref, torch.float32), (px_cur, torch.float32), (status, torch.uint8)):
        assert t.dtype == dt and t.is_cuda and t.is_contiguous()
    assert px_cur.shape == px_ref.shape and status.shape == (n, m) and ref_slot.shape == cur_slot.shape == (n,)
    if error is None:
        error = torch.zeros(n, m, dtype=torch.float32, device=dev)
    params = params or klt_params()
    capi.check(capi.load().svo_hip_klt_track(C.byref(store.layout), store.ptr, n, ref_slot.data_ptr(), cur_slot.data_ptr(), m,
                                             px_ref.data_ptr(), px_cur.data_ptr(), status.data_ptr(), error.data_ptr(),
                                             C.byref(params), _stream_ptr(dev)), "svo_hip_klt_track")
    return error


def klt_summarize(cam, px_ref, px_cur, status):
    """svo_hip_klt_summarize: -> (f_cur [n, m, 3] f64, disparity [n, m] f64, n_tracked [n] i32, median [n] f64)"""
    n, m = px_ref.shape[:2]
    dev = px_ref.device
    f_cur = torch.empty(n, m, 3, dtype=torch.float64, device=dev)
    disparity = torch.empty(n, m, dtype=torch.float64, device=dev)
    n_tracked = torch.empty(n, dtype=torch.int32, device=dev)
    median = torch.empty(n, dtype=torch.float64, device=dev)
    c = capi.camera(cam)
    capi.check(capi.load().svo_hip_klt_summarize(C.byref(c), n, m, px_ref.data_ptr(), px_cur.data_ptr(), status.data_ptr(),
                                                 f_cur.data_ptr(), disparity.data_ptr(), n_tracked.data_ptr(), median.data_ptr(),
                                                 _stream_ptr(dev)), "svo_hip_klt_summarize")
    return f_cur, disparity, n_tracked, median


def homography_params(**kw) -> capi.HomographyParams:
    p = capi.HomographyParams()
    capi.check(capi.load().svo_hip_homography_params_default(C.byref(p)), "svo_hip_homography_params_default")
    for k, v in kw.items():
        if not hasattr(p, k):
            raise capi.SvoHipError(f"svo_hip_homography_params has no field {k}")
        setattr(p, k, v)
    return p


_HOMOGRAPHY_DTYPES = dict(H=torch.float64, best_hypothesis=torch.int32, n_inliers_H=torch.int32, inlier_H=torch.uint8,
                          T_cur_from_ref=torch.float64, ambiguous=torch.int32, status=torch.int32, xyz_in_cur=torch.float64,
                          inlier=torch.uint8, n_inliers=torch.int32, depth_median=torch.float64, scale=torch.float64,
                          T_cur_w=torch.float64, point_w=torch.float64, point_ok=torch.uint8, result=torch.int32)


def homography_outputs(n: int, m: int, device) -> dict:
    """The tensors of svo_hip_homography_out for n pairs of m points, by field name (without the d_ prefix).  Allocate
    once and hand them to every homography_init call that is captured into a HIP graph."""
    shape = dict(H=(n, 9), T_cur_from_ref=(n, 12), T_cur_w=(n, 12), xyz_in_cur=(n, m, 3), point_w=(n, m, 3), inlier_H=(n, m),
                 inlier=(n, m), point_ok=(n, m))
    return {k: torch.zeros(shape.get(k, (n,)), dtype=dt, device=device) for k, dt in _HOMOGRAPHY_DTYPES.items()}


def homography_init(cam, f_ref, f_cur, status, px_ref, px_cur, T_ref_w, params=None, out=None) -> dict:
    """svo_hip_homography_init on tensors: f_ref / f_cur [n, m, 3] f64, status [n, m] u8, px_ref / px_cur [n, m, 2] f32,
    T_ref_w [n, 12] f64 -> dict of the outputs (homography_outputs).  Enqueued on the current stream, not synchronised."""
    n, m = status.shape
    for t, dt, shape in ((f_ref, torch.float64, (n, m, 3)), (f_cur, torch.float64, (n, m, 3)), (status, torch.uint8, (n, m)),
                         (px_ref, torch.float32, (n, m, 2)), (px_cur, torch.float32, (n, m, 2)), (T_ref_w, torch.float64, (n, 12))):
        assert t.dtype == dt and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape
    dev = status.device
    out = homography_outputs(n, m, dev) if out is None else out
    for k, dt in _HOMOGRAPHY_DTYPES.items():
        assert out[k].dtype == dt and out[k].is_contiguous() and out[k].device == dev
    o = capi.HomographyOut(*[out[k].data_ptr() for k in capi.HOMOGRAPHY_OUTPUTS])
    c = capi.camera(cam)
    params = params or homography_params()
    capi.check(capi.load().svo_hip_homography_init(C.byref(c), n, m, f_ref.data_ptr(), f_cur.data_ptr(), status.data_ptr(),
                                                   px_ref.data_ptr(), px_cur.data_ptr(), T_ref_w.data_ptr(), C.byref(params),
                                                   C.byref(o), _stream_ptr(dev)), "svo_hip_homography_init")
    return out


@dataclass
class FirstMap:
    """The tracking-ready state after the bootstrap (svo_hip_first_map, then the detector and svo_hip_initialize_seeds),
    for n sequences of m corners.  Ranks are the reference's inliers_ order; view 0 is the reference frame, view 1 the
    current frame (the next reference of SparseImgAlign: px[:, 1], xyz_ref and n_points are K1's inputs as they are)."""
    n_points: torch.Tensor     # [n] i32
    src_index: torch.Tensor    # [n, m] i32 rank -> corner index, -1 beyond n_points
    pos: torch.Tensor          # [n, m, 3] f64 Point::pos_
    px: torch.Tensor           # [n, 2, m, 2] f64 Feature::px per view
    f: torch.Tensor            # [n, 2, m, 3] f64 Feature::f per view
    key_pts: torch.Tensor      # [n, 2, 5] i32 ranks of Frame::key_pts_, -1 = NULL
    depth_mean: torch.Tensor   # [n] f64 getSceneDepth of the current frame
    depth_min: torch.Tensor    # [n] f64
    xyz_ref: torch.Tensor      # [n, m, 3] f64
    occupancy: torch.Tensor    # [n, cells] u8 setExistingFeatures of the current frame
    seed_ftr: FeatureSet | None = None   # [n, cells(, .)] the new corners of the second keyframe, n_seeds per sequence
    seeds: SeedSet | None = None         # [n, cells] their svo::Seed state
    n_seeds: torch.Tensor | None = None  # [n] i32


_FIRST_MAP_DTYPES = dict(n_points=torch.int32, src_index=torch.int32, pos=torch.float64, px=torch.float64, f=torch.float64,
                         key_pts=torch.int32, depth_mean=torch.float64, depth_min=torch.float64, xyz_ref=torch.float64,
                         occupancy=torch.uint8)


def first_map_outputs(n: int, m: int, cells: int, device) -> FirstMap:
    """The tensors of svo_hip_first_map_out.  Allocate once and hand them to every call that a HIP graph captures."""
    shape = dict(src_index=(n, m), pos=(n, m, 3), px=(n, 2, m, 2), f=(n, 2, m, 3), key_pts=(n, 2, 5), xyz_ref=(n, m, 3),
                 occupancy=(n, cells))
    return FirstMap(**{k: torch.zeros(shape.get(k, (n,)), dtype=dt, device=device) for k, dt in _FIRST_MAP_DTYPES.items()})


def first_map(cam, result, point_ok, point_w, px_ref, px_cur, f_ref, f_cur, T_ref_w, T_cur_w, cell_size: int, grid_n_cols: int,
              grid_n_rows: int, out: FirstMap | None = None) -> FirstMap:
    """svo_hip_first_map on tensors: result [n] i32, point_ok [n, m] u8, point_w / f_ref / f_cur [n, m, 3] f64, px_ref /
    px_cur [n, m, 2] f32, T_ref_w / T_cur_w [n, 12] f64.  Enqueued on the current stream, not synchronised."""
    n, m = point_ok.shape
    for t, dt, shape in ((result, torch.int32, (n,)), (point_ok, torch.uint8, (n, m)), (point_w, torch.float64, (n, m, 3)),
                         (px_ref, torch.float32, (n, m, 2)), (px_cur, torch.float32, (n, m, 2)), (f_ref, torch.float64, (n, m, 3)),
                         (f_cur, torch.float64, (n, m, 3)), (T_ref_w, torch.float64, (n, 12)), (T_cur_w, torch.float64, (n, 12))):
        assert t.dtype == dt and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape
    dev = point_ok.device
    cells = grid_n_cols * grid_n_rows
    out = first_map_outputs(n, m, cells, dev) if out is None else out
    for k, dt in _FIRST_MAP_DTYPES.items():
        t = getattr(out, k)
        assert t.dtype == dt and t.is_contiguous() and t.device == dev
    assert tuple(out.occupancy.shape) == (n, cells) and tuple(out.src_index.shape) == (n, m)
    o = capi.FirstMapOut(*[getattr(out, k).data_ptr() for k in capi.FIRST_MAP_OUTPUTS])
    c = capi.camera(cam)
    capi.check(capi.load().svo_hip_first_map(C.byref(c), n, m, result.data_ptr(), point_ok.data_ptr(), point_w.data_ptr(),
                                             px_ref.data_ptr(), px_cur.data_ptr(), f_ref.data_ptr(), f_cur.data_ptr(),
                                             T_ref_w.data_ptr(), T_cur_w.data_ptr(), cell_size, grid_n_cols, grid_n_rows, cells,
                                             C.byref(o), _stream_ptr(dev)), "svo_hip_first_map")
    return out


class KltTracker:
    """KltHomographyInit up to computeHomography, for n sequences at once.  The defaults are the reference's Config
    values (gridSize 30, nPyrLevels 3, initMinTracked 50, initMinDisparity 50, triangMinCornerScore 20)."""

    MIN_FIRST_FRAME_CORNERS = 100   # initialization.cpp:33

    def __init__(self, cam, grid_size: int = 30, n_pyr_levels: int = 3, min_tracked: int = 50, min_disparity: float = 50.0,
                 min_corner_score: float = 20.0):
        self.cam = cam
        self.min_tracked = min_tracked
        self.min_disparity = min_disparity
        self.min_corner_score = min_corner_score
        self.detector = FastDetector(cam.width, cam.height, grid_size, n_pyr_levels)
        self.params = klt_params()
        self.ref_slots = None

    def add_first_frame(self, store: PyramidStore, slots: torch.Tensor) -> torch.Tensor:
        """addFirstFrame (:29-41) -> [n] InitResult values (i32): SUCCESS, or FAILURE with fewer than 100 corners.
        Sets px_ref [n, cells, 2] f32 (cell order, as detectFeatures fills px_vec), status (the validity mask: 1 where
        the cell holds a corner), px_cur = px_ref, f_ref [n, cells, 3]."""
        if store.n_levels <= self.params.max_level:
            raise capi.SvoHipError(f"the tracker reads pyramid levels 0..{self.params.max_level}: the store has {store.n_levels}")
        xy, level, score = self.detector.detect(store, slots, self.min_corner_score)
        n, cells = score.shape
        self.ref_slots = slots.clone()
        self.status = (level >= 0).to(torch.uint8).contiguous()    # K7's rule: a cell holds a corner iff level >= 0
        self.px_ref = xy.to(torch.float32).contiguous()            # cv::Point2f(ftr->px[0], ftr->px[1])
        self.px_cur = self.px_ref.clone()
        self.f_ref = cam2world(self.cam, xy.to(torch.float64).reshape(-1, 2)).reshape(n, cells, 3)
        self.f_ref = self.f_ref * self.status[..., None].to(torch.float64)
        self.f_cur = torch.zeros_like(self.f_ref)
        self.disparities = torch.zeros(n, cells, dtype=torch.float64, device=store.device)
        self.error = torch.zeros(n, cells, dtype=torch.float32, device=store.device)
        self.n_tracked = self.status.sum(dim=1, dtype=torch.int32)
        self.median_disparity = torch.zeros(n, dtype=torch.float64, device=store.device)
        ok = self.n_tracked >= self.MIN_FIRST_FRAME_CORNERS
        return torch.where(ok, int(InitResult.SUCCESS), int(InitResult.FAILURE)).to(torch.int32)

    def add_frame(self, store: PyramidStore, slots: torch.Tensor) -> torch.Tensor:
        """trackKlt and the gates of addSecondFrame (:45-54) -> [n] InitResult values: FAILURE (fewer than min_tracked
        points left), NO_KEYFRAME (median disparity below min_disparity) or TRACKED.  px_cur and status carry over to
        the next call like px_cur_ and the erased vectors."""
        if self.ref_slots is None:
            raise capi.SvoHipError("add_first_frame has not been called")
        assert slots.dtype == torch.int32 and slots.shape == self.ref_slots.shape
        klt_track(store, self.ref_slots, slots.contiguous(), self.px_ref, self.px_cur, self.status, self.error, self.params)
        self.f_cur, self.disparities, self.n_tracked, self.median_disparity = klt_summarize(self.cam, self.px_ref, self.px_cur, self.status)
        res = torch.full_like(self.n_tracked, int(InitResult.TRACKED))
        res = torch.where(self.median_disparity < self.min_disparity, int(InitResult.NO_KEYFRAME), res)
        res = torch.where(self.n_tracked < self.min_tracked, int(InitResult.FAILURE), res)
        return res


class KltHomographyInit(KltTracker):
    """KltHomographyInit for n sequences at once: KltTracker's addFirstFrame and gates, then svo_hip_homography_init for
    every sequence.  `homography` takes fields of svo_hip_homography_params (reproj_thresh = poseOptimThresh,
    min_inliers = initMinInliers, map_scale = mapScale, n_hypotheses, refine_iters, seed)."""

    def __init__(self, cam, homography: dict | None = None, **tracker):
        super().__init__(cam, **tracker)
        self.homography_params = homography_params(**(homography or {}))
        self.T_ref_w = None
        self.out = None
        self.result = None

    def add_first_frame(self, store: PyramidStore, slots: torch.Tensor, T_ref_w: torch.Tensor | None = None) -> torch.Tensor:
        """addFirstFrame; T_ref_w [n, 12] f64 is frame_ref_->T_f_w_ (identity when omitted)."""
        res = super().add_first_frame(store, slots)
        n = slots.shape[0]
        if T_ref_w is None:
            T_ref_w = torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=torch.float64, device=store.device).repeat(n, 1)
        assert T_ref_w.dtype == torch.float64 and tuple(T_ref_w.shape) == (n, 12)
        self.T_ref_w = T_ref_w.contiguous()
        self.out = None
        self.result = None
        return res

    def add_second_frame(self, store: PyramidStore, slots: torch.Tensor) -> torch.Tensor:
        """addSecondFrame (:43-99) -> [n] InitResult values: FAILURE (too few tracked points, no homography, or too few
        inliers), NO_KEYFRAME (median disparity below min_disparity) or SUCCESS.  Sequences that do not pass the gates
        enter the homography step with every point lost, so their outputs are the entry's zeros."""
        gate = self.add_frame(store, slots)
        tracked = gate == int(InitResult.TRACKED)
        status = (self.status * tracked[:, None].to(torch.uint8)).contiguous()
        n, m = status.shape
        if self.out is None or self.out["inlier"].shape != (n, m):
            self.out = homography_outputs(n, m, store.device)
        homography_init(self.cam, self.f_ref, self.f_cur, status, self.px_ref, self.px_cur, self.T_ref_w, self.homography_params, self.out)
        self.result = torch.where(tracked, self.out["result"], gate)
        return self.result

    def first_map(self, store: PyramidStore, slots: torch.Tensor, frame_index: torch.Tensor | None = None, batch_id: int = 1,
                  out: FirstMap | None = None) -> FirstMap:
        """What processSecondFrame does with the SUCCESS of add_second_frame (frame_handler_mono.cpp:103-127), for every
        sequence: the map, the features and key points of both keyframes, the scene depth and K1's inputs
        (svo_hip_first_map); FAST on the free cells of `slots` (the current frames); a seed per new corner
        (svo_hip_initialize_seeds with depth_mean and 0.5 * depth_min, as addKeyframe is called).  frame_index [n] i32 is
        what the new features' `frame` holds (the sequence number when omitted), batch_id the value of
        Seed::batch_counter after its increment.  `out`: a FirstMap of an earlier call to write into (HIP graphs).
        Sequences without SUCCESS get an empty map; their seeds come from a scene depth of 0.  Everything is enqueued on
        the current stream; nothing is read back."""
        if self.out is None:
            raise capi.SvoHipError("add_second_frame has not been called")
        det = self.detector
        fm = first_map(self.cam, self.result, self.out["point_ok"], self.out["point_w"], self.px_ref, self.px_cur, self.f_ref,
                       self.f_cur, self.T_ref_w, self.out["T_cur_w"], det.cell_size, det.grid_n_cols, det.grid_n_rows, out)
        xy, level, score = det.detect(store, slots, self.min_corner_score, fm.occupancy)
        if frame_index is None:
            frame_index = torch.arange(slots.shape[0], dtype=torch.int32, device=store.device)
        reuse = (fm.seed_ftr, fm.seeds, fm.n_seeds) if fm.seeds is not None else None
        fm.seed_ftr, fm.seeds, fm.n_seeds = DepthFilter.initialize_seeds(self.cam, xy, level, score, self.min_corner_score, frame_index,
                                                                         fm.depth_mean, fm.depth_min * 0.5, batch_id, out=reuse)
        return fm

    # what the reference's members hold after addSecondFrame, for every sequence
    T_cur_from_ref = property(lambda self: self.out["T_cur_from_ref"])   # [n, 12]
    T_f_w = property(lambda self: self.out["T_cur_w"])                   # frame_cur->T_f_w_ [n, 12]
    inliers = property(lambda self: self.out["inlier"])                  # [n, cells] u8 mask (inliers_ as indices in the reference)
    n_inliers = property(lambda self: self.out["n_inliers"])
    xyz_in_cur = property(lambda self: self.out["xyz_in_cur"])           # [n, cells, 3], 0 where not an inlier
    points = property(lambda self: self.out["point_w"])                  # [n, cells, 3] Point::pos_ of the new map points
    point_ok = property(lambda self: self.out["point_ok"])               # [n, cells] u8: the inliers that become map points
    scale = property(lambda self: self.out["scale"])
    ambiguous = property(lambda self: self.out["ambiguous"])
    H = property(lambda self: self.out["H"])
    homography_status = property(lambda self: self.out["status"])
