// pose_common.h -- what the two K4 kernels (pose_optimizer_wave.hip: one wave per frame, what the pipeline runs;
// pose_optimizer.hip: the bit-ordered checker and fix-up kernel, and the four C entries) share: the argument block, the row
// limits, the constants and rules of the reference both restate, the codes of `ran` and the lines that report a finished frame.
#pragma once
#include "capi_common.h"

namespace svo_track {

// The longest row the wave kernel takes (four trips of 64 slots: its radix select keeps a key per trip and lane in registers) and
// the longest the ordered kernel takes (the entries answer SVO_HIP_ERANGE beyond).  A row between the two runs the ordered kernel
// whatever the entry.
constexpr int POSE_WAVE_MAX_STRIDE = 256;
constexpr int PO_MAXN = 1024;

// ran[b] (include/svo_hip.h, d_ran)
constexpr int32_t POSE_RAN_NONE = SVO_HIP_POSE_RAN_NONE;          // no observation had a point: nothing else is written (:57-58)
constexpr int32_t POSE_RAN_DONE = SVO_HIP_POSE_RAN_DONE;          // refined: pose, covariance, flags and statistics are the frame's
constexpr int32_t POSE_RAN_ORDERED = SVO_HIP_POSE_RAN_ORDERED;    // left to the ordered kernel by the wave kernel, untouched

// One block for both kernels and all four entries (pose_optimize_impl fills it).  The wave kernel reads every field.  The
// ordered kernels work in place on has_point / T and read cam.fx, B (pose_opt_flagged_kernel's scan stops there), n, n_stride,
// f, level, pos, has_point, reproj_thresh, n_iter, T, Cov, stats and ran: everything but has_point_in and T_in.
struct PoseArgs {
  svo_hip_camera cam;
  int B;
  const int32_t* n;
  int n_stride;
  const double* f;
  const int32_t* level;
  const double* pos;
  const uint8_t* has_point_in;  // the flags and the pose as the caller has them; == has_point / T: in place
  uint8_t* has_point;           // out: every byte of every row (slots >= n: as they came in)
  double reproj_thresh;
  int n_iter;
  const double* T_in;
  double* T;                    // out: written on every exit (T_in where the kernel leaves the pose alone)
  double* Cov;
  double* stats;
  int32_t* ran;
};

// pose_optimizer_wave.hip: n_stride <= POSE_WAVE_MAX_STRIDE (dynamic LDS: 45 bytes per slot and wave)
int launch_pose_wave(const PoseArgs& a, hipStream_t s);

constexpr double SVO_EPS = 0.0000000001;      // svo/include/svo/global.h:77
constexpr float POSE_MAD_NORMALISER = 1.48f;  // vk::robust_cost::MADScaleEstimator::compute: 1.48 * median(|e|)

// vk::robust_cost::TukeyWeightFunction::value
__device__ __forceinline__ float pose_tukey_weight(float x) {
  const float b_square = 4.6851f * 4.6851f;
  const float x_square = x * x;
  const float tmp = 1.0f - x_square / b_square;
  return (x_square <= b_square) ? tmp * tmp : 0.0f;
}

// The observations of a row from its word of `n` (n_b = a.n[b]; the wave kernel hands it over as a scalar).  Contract:
// n <= n_stride (svo_hip.h); never index past the row.
__device__ __forceinline__ int pose_row_n(const PoseArgs& a, int n_b) { return n_b < 0 ? 0 : (n_b > a.n_stride ? a.n_stride : n_b); }

// Positions of the per-observation arrays both kernels carve out of dynamic LDS: n_stride rounded up to 8, so that every array
// behind an array of doubles starts 8-byte aligned.
__host__ __device__ constexpr int pose_cap(int n_stride) { return (n_stride + 7) & ~7; }

// What a refined frame reports (one lane calls): estimated_scale, error_init, error_final in pixels (:147-152), the observations
// that kept their point (n_err went in, n_deleted were pruned), and ran.  chi2_vec_init is empty without an iteration:
// error_init = 0.
__device__ __forceinline__ void pose_write_result(const PoseArgs& a, int b, double focal, double estimated_scale, double med_init,
                                                  double med_final, int n_err, int n_deleted) {
  a.stats[4 * b + 0] = estimated_scale * focal;
  a.stats[4 * b + 1] = a.n_iter > 0 ? sqrt(med_init) * focal : 0.0;
  a.stats[4 * b + 2] = sqrt(med_final) * focal;
  a.stats[4 * b + 3] = (double)(n_err - n_deleted);
  a.ran[b] = POSE_RAN_DONE;
}

}  // namespace svo_track
