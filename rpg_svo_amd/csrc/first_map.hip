// first_map.hip -- K10: from the bootstrap's point cloud to the state tracking starts from, on the device.
//
// Replaces what FrameHandlerMono::processSecondFrame does after KltHomographyInit::addSecondFrame returns SUCCESS
// (svo/src/frame_handler_mono.cpp:103-127): the Point / Feature pairs in list order (initialization.cpp:78-97),
// setKeyframe() on both frames (Frame::setKeyPoints / checkKeyPoints, frame.cpp:72-126), frame_utils::getSceneDepth
// (frame.cpp:167-188), AbstractDetector::setExistingFeatures (feature_detection.cpp:42-49), the xyz_ref of the next
// sparse alignment (sparse_img_align.cpp:107-108) and, after the detector has run, the Seed of every new corner
// (DepthFilter::initializeSeeds, depth_filter.cpp:37-46, 114-132).  include/svo_hip.h states both entries;
// tests/first_map_checker.py restates them in sequential numpy loops.
//
//   first_map_kernel   one workgroup of 256 work-items per sequence.  The point_ok corners are compacted in index
//                      order (block_select.h's block_compact_step, which K9 uses too); rank -> corner
//                      index and the depth of every rank stay in LDS (12 KB).  One work-item per rank copies the map
//                      point and its two features and forms its depth, xyz_ref and grid cell.  The ten key points
//                      (five per view) and the minimum depth are arg-max / arg-min reductions on integers: the value
//                      as an order-preserving 64-bit key through an LDS atomicMax, then the smallest rank that holds
//                      the winning key through an LDS atomicMin -- "strictly better replaces" of the sequential scan
//                      is "the best value, ties to the smallest rank".  No floating-point atomics: the same call gives
//                      the same bits, and so do identical sequences wherever they stand in the batch.  The median
//                      depth is block_select.h's block_rank_select.
//   seed_init_kernel   one workgroup of 256 per keyframe: the cells with a corner are compacted in cell order, in blocks
//                      of 256 cells with a running offset; one work-item per new seed.
#pragma clang fp contract(off)
#include "block_select.h"
#include "capi_common.h"
#include "frame_keys.h"
#include "track_math.h"

using namespace svo_capi;
using namespace svo_dev;

namespace {

constexpr int FM_MAX_PTS = 1024;
constexpr int FM_THREADS = 256;
constexpr int FM_KEYS = 10;      // key point k of view v is key 5 v + k

struct FirstMapArgs {
  int n_pts;
  int width, height;
  int cell_size, grid_n_cols, grid_n_rows, cells;
  const int32_t* result;
  const uint8_t* point_ok;
  const double* point_w;
  const float* px_ref;
  const float* px_cur;
  const double* f_ref;
  const double* f_cur;
  const double* T_cur_w;
  svo_hip_first_map_out o;
};

__global__ void __launch_bounds__(FM_THREADS) first_map_kernel(const FirstMapArgs a) {
  __shared__ double s_z[FM_MAX_PTS];               // depth in the current frame, by rank
  __shared__ int s_idx[FM_MAX_PTS];                // rank -> corner index
  __shared__ unsigned long long s_key[FM_KEYS + 1];  // the best key of each key point; [FM_KEYS]: of the minimum depth
  __shared__ int s_first[FM_KEYS];                 // the first member of each key point's set
  __shared__ int s_first_nan[FM_KEYS];             // .. and whether its value is NaN (then nothing ever replaces it)
  __shared__ int s_rank[FM_KEYS];                  // the smallest rank that holds the best key
  __shared__ int s_wcnt[4];
  __shared__ double s_med;
  const int seq = (int)xcd_contiguous_block(), t = (int)threadIdx.x;
  const int n_pts = a.n_pts;
  const size_t base = (size_t)seq * n_pts;
  const svo_hip_first_map_out& o = a.o;
  const bool success = a.result[seq] == SVO_HIP_INIT_SUCCESS;  // (workgroup-uniform)

  if (t < FM_KEYS) key_points_init(s_key, s_first, s_first_nan, s_rank, t);
  if (t == 0) {
    s_key[FM_KEYS] = depth_min_start();
    s_med = 0.0;
  }
  for (int c = t; c < a.cells; c += FM_THREADS) o.d_occupancy[(size_t)seq * a.cells + c] = 0;

  // ---- the point_ok corners in index order: inliers_ with the test of initialization.cpp:84 applied ---------------------
  int m = 0;
  for (int c0 = 0; c0 < n_pts; c0 += FM_THREADS) {
    const int i = c0 + t;
    const bool on = success && i < n_pts && a.point_ok[base + (i < n_pts ? i : 0)] != 0;
    const int j = block_compact_step<FM_THREADS / 64>(on, t, s_wcnt, m);
    if (on) s_idx[j] = i;
  }
  __syncthreads();  // (s_idx, the initial keys and the zeroed occupancy are in place)

  Se3 T_cw;
  double pos_cur[3];
  se3_from_Rt(a.T_cur_w + 12 * (size_t)seq, T_cw);
  frame_pos(T_cw, pos_cur);
  const int cu = a.width / 2, cv = a.height / 2;

  // ---- one work-item per rank: the point, its two features, depth, xyz_ref, cell; the first members -------------------
  for (int j = t; j < n_pts; j += FM_THREADS) {
    const size_t r = base + j;
    double* px_out[2] = {o.d_px + 2 * ((2 * (size_t)seq) * n_pts + j), o.d_px + 2 * ((2 * (size_t)seq + 1) * n_pts + j)};
    double* f_out[2] = {o.d_f + 3 * ((2 * (size_t)seq) * n_pts + j), o.d_f + 3 * ((2 * (size_t)seq + 1) * n_pts + j)};
    if (j >= m) {
      o.d_src_index[r] = -1;
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        o.d_pos[3 * r + e] = 0.0;
        o.d_xyz_ref[3 * r + e] = 0.0;
        f_out[0][e] = 0.0;
        f_out[1][e] = 0.0;
      }
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        px_out[0][e] = 0.0;
        px_out[1][e] = 0.0;
      }
      continue;
    }
    const int i = s_idx[j];  // < n_pts: it is an index the compaction loop visited
    const size_t gi = base + i;
    o.d_src_index[r] = i;
    const double pos[3] = {a.point_w[3 * gi], a.point_w[3 * gi + 1], a.point_w[3 * gi + 2]};
    const double px[2][2] = {{(double)a.px_ref[2 * gi], (double)a.px_ref[2 * gi + 1]},
                             {(double)a.px_cur[2 * gi], (double)a.px_cur[2 * gi + 1]}};
    const double fc[3] = {a.f_cur[3 * gi], a.f_cur[3 * gi + 1], a.f_cur[3 * gi + 2]};
    double in_cur[3];
    se3_apply(T_cw, pos, in_cur);  // frame.w2f(point->pos_)
    s_z[j] = in_cur[2];
    const double dx = pos[0] - pos_cur[0], dy = pos[1] - pos_cur[1], dz = pos[2] - pos_cur[2];
    const double depth = sqrt((dx * dx + dy * dy) + dz * dz);
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      o.d_pos[3 * r + e] = pos[e];
      o.d_xyz_ref[3 * r + e] = fc[e] * depth;
      f_out[0][e] = a.f_ref[3 * gi + e];
      f_out[1][e] = fc[e];
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      px_out[0][e] = px[0][e];
      px_out[1][e] = px[1][e];
    }
    // setExistingFeatures of the current frame
    occupancy_mark(o.d_occupancy + (size_t)seq * a.cells, px[1][0], px[1][1], a.cell_size, a.grid_n_cols, a.grid_n_rows);
#pragma unroll
    for (int v = 0; v < 2; ++v) key_points_first(key_values(px[v][0], px[v][1], cu, cv), j, s_first + 5 * v);
  }
  __syncthreads();

  // ---- the best value of every key point, and the minimum depth ----------------------------------------------------------
  for (int j = t; j < m; j += FM_THREADS) {
    const size_t gi = base + s_idx[j];
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const float* p = (v == 0 ? a.px_ref : a.px_cur) + 2 * gi;
      key_points_best(key_values((double)p[0], (double)p[1], cu, cv), j, s_key + 5 * v, s_first + 5 * v, s_first_nan + 5 * v);
    }
    depth_min_add(&s_key[FM_KEYS], s_z[j]);
  }
  __syncthreads();

  // ---- the smallest rank with that value; the median depth -----------------------------------------------------------------
  for (int j = t; j < m; j += FM_THREADS) {
    const size_t gi = base + s_idx[j];
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const float* p = (v == 0 ? a.px_ref : a.px_cur) + 2 * gi;
      key_points_rank(key_values((double)p[0], (double)p[1], cu, cv), j, s_key + 5 * v, s_rank + 5 * v);
    }
  }
  // vk::getMedian: rank m / 2 of the m depths; a NaN is never smaller or equal, so it has no rank and adds to none
  block_rank_select<FM_THREADS>(s_z, m, m / 2, t, [&](int j) { return s_z[j] == s_z[j]; }, &s_med);
  __syncthreads();

  if (t < FM_KEYS) o.d_key_pts[FM_KEYS * (size_t)seq + t] = key_point_result(s_first, s_first_nan, s_rank, t);
  if (t == 0) {
    o.d_n_points[seq] = m;
    o.d_depth_mean[seq] = m > 0 ? s_med : 0.0;
    o.d_depth_min[seq] = m > 0 ? depth_min_value(&s_key[FM_KEYS]) : 0.0;
  }
}

struct SeedInitArgs {
  Cam cam;
  int n_cells, seed_stride;
  const int32_t* corner_xy;
  const int32_t* corner_level;
  const float* corner_score;
  double detection_threshold;
  const int32_t* frame_index;
  const double* depth_mean;
  const double* depth_min;
  int batch_id;
  svo_hip_seed_init_out o;
};

__global__ void __launch_bounds__(FM_THREADS) seed_init_kernel(const SeedInitArgs a) {
  __shared__ int s_wcnt[4];
  const int frame = (int)xcd_contiguous_block(), t = (int)threadIdx.x;
  const size_t in0 = (size_t)frame * a.n_cells, out0 = (size_t)frame * a.seed_stride;
  const svo_hip_seed_init_out& o = a.o;
  // Seed(ftr, float depth_mean, float depth_min): the arguments are floats, the divisions are doubles
  const float depth_mean = (float)a.depth_mean[frame], depth_min = (float)a.depth_min[frame];
  const float mu = (float)(1.0 / (double)depth_mean);
  const float z_range = (float)(1.0 / (double)depth_min);
  const float sigma2 = z_range * z_range / 36;
  const int frame_index = a.frame_index[frame];

  int n = 0;  // the running offset: seeds of the blocks before this one
  for (int c0 = 0; c0 < a.n_cells; c0 += FM_THREADS) {
    const int c = c0 + t;
    // (an empty cell holds level -1 and (float)threshold, which can lie above the double: the level decides)
    const size_t ci = in0 + (c < a.n_cells ? c : 0);
    const bool on = c < a.n_cells && a.corner_level[ci] >= 0 && (double)a.corner_score[ci] > a.detection_threshold;
    const int slot = block_compact_step<FM_THREADS / 64>(on, t, s_wcnt, n);
    if (on) {
      const size_t s = out0 + slot;  // at most c: inside the frame's stride
      const double px[2] = {(double)a.corner_xy[2 * (in0 + c)], (double)a.corner_xy[2 * (in0 + c) + 1]};
      double f[3];
      cam2world(a.cam, px[0], px[1], f);  // Feature(frame, px, level), feature.h:42-50
      o.d_frame[s] = frame_index;
      o.d_level[s] = a.corner_level[in0 + c];
      o.d_px[2 * s] = px[0];
      o.d_px[2 * s + 1] = px[1];
      o.d_f[3 * s] = f[0];
      o.d_f[3 * s + 1] = f[1];
      o.d_f[3 * s + 2] = f[2];
      if (o.d_type) o.d_type[s] = SVO_HIP_FTR_CORNER;
      if (o.d_grad) {
        o.d_grad[2 * s] = 1.0;
        o.d_grad[2 * s + 1] = 0.0;
      }
      o.d_a[s] = 10.0f;
      o.d_b[s] = 10.0f;
      o.d_mu[s] = mu;
      o.d_z_range[s] = z_range;
      o.d_sigma2[s] = sigma2;
      o.d_batch_id[s] = a.batch_id;
    }
  }
  if (t == 0) o.d_n_seeds[frame] = n;
  for (int j = n + t; j < a.seed_stride; j += FM_THREADS) {
    const size_t s = out0 + j;
    o.d_frame[s] = 0;
    o.d_level[s] = 0;
    o.d_px[2 * s] = 0.0;
    o.d_px[2 * s + 1] = 0.0;
    o.d_f[3 * s] = 0.0;
    o.d_f[3 * s + 1] = 0.0;
    o.d_f[3 * s + 2] = 0.0;
    if (o.d_type) o.d_type[s] = 0;
    if (o.d_grad) {
      o.d_grad[2 * s] = 0.0;
      o.d_grad[2 * s + 1] = 0.0;
    }
    o.d_a[s] = 0.0f;
    o.d_b[s] = 0.0f;
    o.d_mu[s] = 0.0f;
    o.d_z_range[s] = 0.0f;
    o.d_sigma2[s] = 0.0f;
    o.d_batch_id[s] = 0;
  }
}

}  // namespace

extern "C" {

int svo_hip_first_map(const svo_hip_camera* cam, int n_seq, int n_pts, const int32_t* d_result, const uint8_t* d_point_ok,
                      const double* d_point_w, const float* d_px_ref, const float* d_px_cur, const double* d_f_ref,
                      const double* d_f_cur, const double* d_T_ref_w, const double* d_T_cur_w, int cell_size, int grid_n_cols,
                      int grid_n_rows, int cells, const svo_hip_first_map_out* out, void* stream) {
  if (!cam || !out || n_seq < 0 || n_pts < 0 || cell_size <= 0 || grid_n_cols < 0 || grid_n_rows < 0 || cells < 0) return SVO_HIP_EINVAL;
  if ((int64_t)grid_n_cols * grid_n_rows != (int64_t)cells) return SVO_HIP_EINVAL;
  if (n_pts > FM_MAX_PTS) return SVO_HIP_ERANGE;
  if ((int64_t)n_seq * n_pts == 0) return SVO_HIP_OK;
  if ((int64_t)n_seq * n_pts > 0x7fffffff || (int64_t)n_seq * cells > 0x7fffffff) return SVO_HIP_ERANGE;
  if (!d_result || !d_point_ok || !d_point_w || !d_px_ref || !d_px_cur || !d_f_ref || !d_f_cur || !d_T_ref_w || !d_T_cur_w)
    return SVO_HIP_EINVAL;
  if (!out->d_n_points || !out->d_src_index || !out->d_pos || !out->d_px || !out->d_f || !out->d_key_pts || !out->d_depth_mean ||
      !out->d_depth_min || !out->d_xyz_ref || !out->d_occupancy)
    return SVO_HIP_EINVAL;
  FirstMapArgs a;
  a.n_pts = n_pts;
  a.width = cam->width; a.height = cam->height;
  a.cell_size = cell_size; a.grid_n_cols = grid_n_cols; a.grid_n_rows = grid_n_rows; a.cells = cells;
  a.result = d_result; a.point_ok = d_point_ok; a.point_w = d_point_w; a.px_ref = d_px_ref; a.px_cur = d_px_cur;
  a.f_ref = d_f_ref; a.f_cur = d_f_cur; a.T_cur_w = d_T_cur_w;
  a.o = *out;
  hipLaunchKernelGGL(first_map_kernel, dim3((unsigned)n_seq), dim3(FM_THREADS), 0, static_cast<hipStream_t>(stream), a);
  return check_launch();
}

int svo_hip_initialize_seeds(const svo_hip_camera* cam, int n_frames, int n_cells, const int32_t* d_corner_xy,
                             const int32_t* d_corner_level, const float* d_corner_score, double detection_threshold,
                             const int32_t* d_frame_index, const double* d_depth_mean, const double* d_depth_min, int batch_id,
                             int seed_stride, const svo_hip_seed_init_out* out, void* stream) {
  if (!cam || !cam_model_ok(cam) || !out || n_frames < 0 || n_cells < 0 || seed_stride < n_cells) return SVO_HIP_EINVAL;
  if (n_frames == 0) return SVO_HIP_OK;
  if ((int64_t)n_frames * seed_stride > 0x7fffffff) return SVO_HIP_ERANGE;
  if (!d_frame_index || !d_depth_mean || !d_depth_min || !out->d_n_seeds) return SVO_HIP_EINVAL;
  if (n_cells > 0 && (!d_corner_xy || !d_corner_level || !d_corner_score)) return SVO_HIP_EINVAL;
  if (seed_stride > 0 && (!out->d_frame || !out->d_level || !out->d_px || !out->d_f || !out->d_a || !out->d_b || !out->d_mu ||
                          !out->d_z_range || !out->d_sigma2 || !out->d_batch_id))
    return SVO_HIP_EINVAL;
  SeedInitArgs a;
  a.cam = make_cam(cam);
  a.n_cells = n_cells; a.seed_stride = seed_stride;
  a.corner_xy = d_corner_xy; a.corner_level = d_corner_level; a.corner_score = d_corner_score;
  a.detection_threshold = detection_threshold;
  a.frame_index = d_frame_index; a.depth_mean = d_depth_mean; a.depth_min = d_depth_min;
  a.batch_id = batch_id;
  a.o = *out;
  hipLaunchKernelGGL(seed_init_kernel, dim3((unsigned)n_frames), dim3(FM_THREADS), 0, static_cast<hipStream_t>(stream), a);
  return check_launch();
}

}  // extern "C"
