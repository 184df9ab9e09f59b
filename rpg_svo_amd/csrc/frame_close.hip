// frame_close.hip -- K11: the end of a tracked frame, on the device.
//
// Replaces what FrameHandlerMono::processFrame does after the reprojector and the pose optimizer have run
// (svo/src/frame_handler_mono.cpp:151-193, 224-229, 304-315): the three failure gates with setTrackingQuality
// (frame_handler_base.cpp:157-171), frame_utils::getSceneDepth (frame.cpp:167-188), needNewKf, setKeyframe()
// (Frame::setKeyPoints / checkKeyPoints, frame.cpp:72-126), AbstractDetector::setExistingFeatures
// (feature_detection.cpp:42-49), Map::getFurthestKeyframe (map.cpp:149-162) and the xyz_ref / visibility of the next sparse
// alignment (sparse_img_align.cpp:102-108).  include/svo_hip.h states the entry; tests/frame_close_checker.py restates it in
// sequential loops.
//
//   frame_close_kernel  one workgroup of 256 work-items per sequence.  The gates are scalar work every work-item repeats
//                       (workgroup-uniform).  One work-item per row forms its depth (kept in LDS, 8 KB), xyz_ref, valid and
//                       grid cell; there is no compaction -- the key points are row indices, and the rows without a point
//                       are simply no members.  Key points and minimum depth are frame_keys.h's reductions on integers
//                       (K10's), the median depth is block_select.h's block_rank_select over the rows with a point.  One
//                       work-item per keyframe then tests needNewKf's box (smallest blocking index: LDS atomicMin) and
//                       forms its distance for getFurthestKeyframe (order-preserving key: atomicMax, then atomicMin of the
//                       index).  No floating-point atomics: the same call gives the same bits, and so do identical
//                       sequences wherever they stand in the batch.
#pragma clang fp contract(off)
#include "block_select.h"
#include "capi_common.h"
#include "frame_keys.h"
#include "track_math.h"

using namespace svo_capi;
using namespace svo_dev;

namespace {

constexpr int FC_MAX_ROWS = 1024;
constexpr int FC_MAX_KFS = 64;
constexpr int FC_THREADS = 256;

struct FrameCloseArgs {
  int n_stride, kf_stride;
  int width, height;
  int cell_size, grid_n_cols, grid_n_rows, cells;
  svo_hip_frame_close_params p;
  svo_hip_frame_close_in in;
  svo_hip_frame_close_out o;
};

__global__ void __launch_bounds__(FC_THREADS) frame_close_kernel(const FrameCloseArgs a) {
  __shared__ double s_z[FC_MAX_ROWS];          // depth in the frame, by row (rows with a point)
  __shared__ unsigned char s_on[FC_MAX_ROWS];  // the row has a point
  __shared__ unsigned long long s_key[5 + 2];  // key points; [5]: minimum depth; [6]: largest keyframe distance
  __shared__ int s_first[5], s_first_nan[5], s_rank[5];
  __shared__ int s_cnt;                        // rows with a point
  __shared__ int s_block, s_far;
  __shared__ double s_med;
  const int seq = (int)xcd_contiguous_block(), t = (int)threadIdx.x;
  const svo_hip_frame_close_in& in = a.in;
  const svo_hip_frame_close_out& o = a.o;
  const size_t base = (size_t)seq * a.n_stride;
  int n = in.d_n[seq];
  n = n < 0 ? 0 : (n > a.n_stride ? a.n_stride : n);
  int n_kf = in.d_n_kf[seq];
  n_kf = n_kf < 0 ? 0 : (n_kf > a.kf_stride ? a.kf_stride : n_kf);

  // ---- the gates (frame_handler_mono.cpp:151, :170; setTrackingQuality, frame_handler_base.cpp:157-171) ---------------
  const int num_obs = in.d_num_obs[seq], num_obs_last = in.d_num_obs_last[seq];
  int gate = 0;
  if (n < a.p.quality_min_fts) gate = 1;
  else if (num_obs < a.p.min_pose_obs) gate = 2;
  else {
    const int drop = (num_obs_last < a.p.max_fts ? num_obs_last : a.p.max_fts) - num_obs;  // int(std::min(last, maxFts)) - n
    if (num_obs < a.p.quality_min_fts || drop > a.p.quality_max_drop_fts) gate = 3;
  }
  const double* T_sel = (gate == 1 || gate == 3) ? in.d_T_last + 12 * (size_t)seq : in.d_T_f_w + 12 * (size_t)seq;

  if (t < 5) key_points_init(s_key, s_first, s_first_nan, s_rank, t);
  if (t == 0) {
    s_key[5] = depth_min_start();
    s_key[6] = 0ull;
    s_cnt = 0;
    s_block = KEY_NONE;
    s_far = KEY_NONE;
    s_med = 0.0;
  }
  if (t < 12) o.d_T_out[12 * (size_t)seq + t] = T_sel[t];
  for (int c = t; c < a.cells; c += FC_THREADS) o.d_occupancy[(size_t)seq * a.cells + c] = 0;
  __syncthreads();  // (the initial keys and the zeroed occupancy are in place)

  Se3 T;
  double pos_f[3];
  se3_from_Rt(T_sel, T);
  frame_pos(T, pos_f);
  const int cu = a.width / 2, cv = a.height / 2;

  // ---- one work-item per row: valid, depth, xyz_ref, cell; the first members ------------------------------------------------
  for (int j = t; j < a.n_stride; j += FC_THREADS) {
    const size_t r = base + j;
    const bool row = j < n;
    const bool on = row && in.d_has_point[r] != 0;
    s_on[j] = on ? 1 : 0;
    o.d_valid[r] = on ? 1 : 0;
    if (row)  // setExistingFeatures takes every feature of the frame, with or without a point
      occupancy_mark(o.d_occupancy + (size_t)seq * a.cells, in.d_px[2 * r], in.d_px[2 * r + 1], a.cell_size, a.grid_n_cols, a.grid_n_rows);
    if (!on) {
      s_z[j] = 0.0;
#pragma unroll
      for (int e = 0; e < 3; ++e) o.d_xyz_ref[3 * r + e] = 0.0;
      continue;
    }
    const double pos[3] = {in.d_pos[3 * r], in.d_pos[3 * r + 1], in.d_pos[3 * r + 2]};
    double in_f[3];
    se3_apply(T, pos, in_f);  // frame.w2f(point->pos_)
    s_z[j] = in_f[2];
    const double dx = pos[0] - pos_f[0], dy = pos[1] - pos_f[1], dz = pos[2] - pos_f[2];
    const double depth = sqrt((dx * dx + dy * dy) + dz * dz);
#pragma unroll
    for (int e = 0; e < 3; ++e) o.d_xyz_ref[3 * r + e] = in.d_f[3 * r + e] * depth;
    key_points_first(key_values(in.d_px[2 * r], in.d_px[2 * r + 1], cu, cv), j, s_first);
    atomicAdd(&s_cnt, 1);
  }
  __syncthreads();

  // ---- the best value of every key point, and the minimum depth -----------------------------------------------------------
  for (int j = t; j < n; j += FC_THREADS) {
    if (!s_on[j]) continue;
    const size_t r = base + j;
    key_points_best(key_values(in.d_px[2 * r], in.d_px[2 * r + 1], cu, cv), j, s_key, s_first, s_first_nan);
    depth_min_add(&s_key[5], s_z[j]);
  }
  __syncthreads();

  // ---- the smallest row with that value; the median depth ------------------------------------------------------------------
  for (int j = t; j < n; j += FC_THREADS) {
    if (!s_on[j]) continue;
    const size_t r = base + j;
    key_points_rank(key_values(in.d_px[2 * r], in.d_px[2 * r + 1], cu, cv), j, s_key, s_rank);
  }
  const int m = s_cnt;
  // vk::getMedian: rank m / 2 of the m depths; a NaN is never smaller or equal, so it has no rank and adds to none
  block_rank_select<FC_THREADS>(s_z, n, m / 2, t, [&](int j) { return s_on[j] != 0 && s_z[j] == s_z[j]; }, &s_med);
  __syncthreads();

  const double depth_mean = m > 0 ? s_med : 0.0;

  // ---- one work-item per keyframe: needNewKf's box, and the distance of getFurthestKeyframe -------------------------------
  double dist = 0.0;
  if (t < n_kf) {
    const size_t k = (size_t)seq * a.kf_stride + t;
    Se3 T_kf;
    double kf_pos[3], rel[3];
    se3_from_Rt(in.d_kf_T + 12 * k, T_kf);
    frame_pos(T_kf, kf_pos);
    if (in.d_kf_overlap[k] >= 0) {
      se3_apply(T, kf_pos, rel);  // new_frame_->w2f(kf->pos())
      const double mind = a.p.kfselect_mindist;
      if (fabs(rel[0]) / depth_mean < mind && fabs(rel[1]) / depth_mean < mind * 0.8 && fabs(rel[2]) / depth_mean < mind * 1.3)
        atomicMin(&s_block, t);
    }
    const double dx = kf_pos[0] - pos_f[0], dy = kf_pos[1] - pos_f[1], dz = kf_pos[2] - pos_f[2];
    dist = sqrt((dx * dx + dy * dy) + dz * dz);  // ((*it)->pos() - pos).norm()
    if (dist > 0.0) atomicMax(&s_key[6], ordered_key(dist));  // (false for NaN: it never exceeds maxdist)
  }
  __syncthreads();
  if (t < n_kf && dist > 0.0 && ordered_key(dist) == s_key[6]) atomicMin(&s_far, t);
  __syncthreads();

  if (t < 5) o.d_key_pts[5 * (size_t)seq + t] = key_point_result(s_first, s_first_nan, s_rank, t);
  if (t == 0) {
    const int block = s_block == KEY_NONE ? -1 : s_block;
    const int quality = gate != 0 ? SVO_HIP_TRACKING_INSUFFICIENT : SVO_HIP_TRACKING_GOOD;
    int result = SVO_HIP_RESULT_FAILURE;
    if (gate == 0) result = block >= 0 ? SVO_HIP_RESULT_NO_KEYFRAME : SVO_HIP_RESULT_IS_KEYFRAME;  // (the quality is never TRACKING_BAD)
    o.d_gate[seq] = gate;
    o.d_quality[seq] = quality;
    o.d_result[seq] = result;
    o.d_nobs_out[seq] = m;
    o.d_depth_mean[seq] = depth_mean;
    o.d_depth_min[seq] = m > 0 ? depth_min_value(&s_key[5]) : 0.0;
    o.d_kf_block[seq] = block;
    const bool limited = a.p.max_n_kfs > 2 && n_kf >= a.p.max_n_kfs;  // (frame_handler_mono.cpp:224)
    o.d_kf_remove[seq] = (limited && s_far != KEY_NONE) ? s_far : -1;
  }
}

}  // namespace

extern "C" {

int svo_hip_frame_close_params_default(svo_hip_frame_close_params* out) {
  if (!out) return SVO_HIP_EINVAL;
  out->quality_min_fts = 50;
  out->quality_max_drop_fts = 40;
  out->max_fts = 120;
  out->max_n_kfs = 10;
  out->kfselect_mindist = 0.12;
  out->min_pose_obs = 20;
  out->reserved = 0;
  return SVO_HIP_OK;
}

int svo_hip_frame_close(const svo_hip_camera* cam, int B, int n_stride, int kf_stride, const svo_hip_frame_close_in* in,
                        int cell_size, int grid_n_cols, int grid_n_rows, int cells, const svo_hip_frame_close_params* params,
                        const svo_hip_frame_close_out* out, void* stream) {
  if (!cam || !in || !params || !out || B < 0 || n_stride < 0 || kf_stride < 0 || cell_size <= 0 || grid_n_cols < 0 || grid_n_rows < 0 ||
      cells < 0)
    return SVO_HIP_EINVAL;
  if ((int64_t)grid_n_cols * grid_n_rows != (int64_t)cells) return SVO_HIP_EINVAL;
  if (n_stride > FC_MAX_ROWS || kf_stride > FC_MAX_KFS) return SVO_HIP_ERANGE;
  if (B == 0) return SVO_HIP_OK;
  if ((int64_t)B * n_stride > 0x7fffffff || (int64_t)B * cells > 0x7fffffff) return SVO_HIP_ERANGE;
  if (!in->d_n || !in->d_T_f_w || !in->d_T_last || !in->d_num_obs || !in->d_num_obs_last || !in->d_n_kf) return SVO_HIP_EINVAL;
  if (n_stride > 0 && (!in->d_px || !in->d_f || !in->d_pos || !in->d_has_point || !out->d_valid || !out->d_xyz_ref)) return SVO_HIP_EINVAL;
  if (kf_stride > 0 && (!in->d_kf_T || !in->d_kf_overlap)) return SVO_HIP_EINVAL;
  if (cells > 0 && !out->d_occupancy) return SVO_HIP_EINVAL;
  if (!out->d_gate || !out->d_quality || !out->d_result || !out->d_T_out || !out->d_nobs_out || !out->d_depth_mean ||
      !out->d_depth_min || !out->d_kf_block || !out->d_key_pts || !out->d_kf_remove)
    return SVO_HIP_EINVAL;
  FrameCloseArgs a;
  a.n_stride = n_stride; a.kf_stride = kf_stride;
  a.width = cam->width; a.height = cam->height;
  a.cell_size = cell_size; a.grid_n_cols = grid_n_cols; a.grid_n_rows = grid_n_rows; a.cells = cells;
  a.p = *params;
  a.in = *in;
  a.o = *out;
  hipLaunchKernelGGL(frame_close_kernel, dim3((unsigned)B), dim3(FC_THREADS), 0, static_cast<hipStream_t>(stream), a);
  return check_launch();
}

}  // extern "C"
