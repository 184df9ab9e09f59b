// frame_keys.h -- what a keyframe needs of its feature list, for the kernels that make one (K10 first_map.hip, K11
// frame_close.hip): Frame::checkKeyPoints' five arg-max rules and getSceneDepth's minimum as reductions on integers, and
// the cell of AbstractDetector::setExistingFeatures.  A value becomes an order-preserving 64-bit key; an LDS atomicMax
// finds the best key, then an LDS atomicMin the smallest list index that holds it -- "strictly better replaces" of the
// sequential scan is "the best value, ties to the smallest index".  No floating-point atomics.  The arithmetic here is one
// subtraction, one product and one division per value: nothing a contraction could fuse, so the header does not depend on
// the contraction mode of the including file.
#pragma once
#include <cstddef>
#include <cstdint>
#ifndef SVO_HOST_MATH_TEST  // (see device_math.h)
#include <hip/hip_runtime.h>
#endif

namespace svo_dev {

constexpr int KEY_NONE = 0x7fffffff;

// v -> an unsigned key with the order of the doubles (v is not NaN; -0 and +0 get different keys)
__device__ __forceinline__ unsigned long long ordered_key(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double ordered_value(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

// What checkKeyPoints compares for the feature at (px0, px1): key point k is the member with the LARGEST key[k].
// k = 0 is the feature closest to the centre in the maximum norm, so its key is the complement of the distance's.
// Keys are > 0; a NaN value has no key (nan[k]).  A zero product is +0 whatever its sign: -0 > +0 is false.
struct KeyVals {
  bool member[5], nan[5];
  unsigned long long key[5];
};
__device__ __forceinline__ KeyVals key_values(double px0, double px1, int cu, int cv) {
  KeyVals r;
  const double dx = px0 - (double)cu, dy = px1 - (double)cv;
  const double ax = fabs(dx), ay = fabs(dy);
  const double dist = (ax < ay) ? ay : ax;  // std::max(ax, ay)
  double prod = dx * dy;
  prod = (prod == 0.0) ? 0.0 : prod;
  r.member[0] = true;
  r.member[1] = px0 >= (double)cu && px1 >= (double)cv;
  r.member[2] = px0 >= (double)cu && px1 < (double)cv;
  r.member[3] = px0 < (double)cv && px1 < (double)cv;   // (frame.cpp:110 tests px[0] against cv)
  r.member[4] = px0 < (double)cv && px1 >= (double)cv;  // (frame.cpp:118 likewise)
  r.nan[0] = dist != dist;
  r.key[0] = ~ordered_key(dist);
#pragma unroll
  for (int k = 1; k < 5; ++k) {
    r.nan[k] = prod != prod;
    r.key[k] = ordered_key(prod);
  }
  return r;
}

// The five key points of ONE feature list, in three passes over its members with a workgroup barrier between them.  The
// four arrays are LDS, five entries each, initialised by key_points_init before the barrier that precedes pass 1.
//   pass 1  key_points_first   the first member of each key point's set
//   pass 2  key_points_best    the best key of each set; whether the first member's value is NaN (nothing replaces it then)
//   pass 3  key_points_rank    the smallest index that holds the best key
//   after   key_point_result   -1 for an empty set
__device__ __forceinline__ void key_points_init(unsigned long long* s_key, int* s_first, int* s_first_nan, int* s_rank, int k) {
  s_key[k] = 0ull;
  s_first[k] = KEY_NONE;
  s_first_nan[k] = 0;
  s_rank[k] = KEY_NONE;
}
__device__ __forceinline__ void key_points_first(const KeyVals& kv, int j, int* s_first) {
#pragma unroll
  for (int k = 0; k < 5; ++k)
    if (kv.member[k]) atomicMin(&s_first[k], j);
}
__device__ __forceinline__ void key_points_best(const KeyVals& kv, int j, unsigned long long* s_key, const int* s_first, int* s_first_nan) {
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    if (!kv.member[k]) continue;
    if (!kv.nan[k]) atomicMax(&s_key[k], kv.key[k]);
    else if (s_first[k] == j) s_first_nan[k] = 1;
  }
}
__device__ __forceinline__ void key_points_rank(const KeyVals& kv, int j, const unsigned long long* s_key, int* s_rank) {
#pragma unroll
  for (int k = 0; k < 5; ++k)
    if (kv.member[k] && !kv.nan[k] && kv.key[k] == s_key[k]) atomicMin(&s_rank[k], j);
}
__device__ __forceinline__ int key_point_result(const int* s_first, const int* s_first_nan, const int* s_rank, int k) {
  const int first = s_first[k];
  return first == KEY_NONE ? -1 : (s_first_nan[k] ? first : s_rank[k]);
}

// getSceneDepth's depth_min = fmin over the depths from numeric_limits<double>::max(), as the largest complemented key:
// *s_key starts at depth_min_start(), every depth goes through depth_min_add (fmin skips a NaN), depth_min_value reads it.
__device__ __forceinline__ unsigned long long depth_min_start() { return ~ordered_key(1.7976931348623157e308); }
__device__ __forceinline__ void depth_min_add(unsigned long long* s_key, double z) {
  if (z == z) atomicMax(s_key, ~ordered_key(z));
}
__device__ __forceinline__ double depth_min_value(const unsigned long long* s_key) { return ordered_value(~*s_key); }

// setExistingFeatures for one pixel: occupancy[int(px1 / cell_size) * grid_n_cols + int(px0 / cell_size)] = 1.  A cell
// index is used only after it is known to lie inside the grid: a pixel that is not finite, or whose row / column lies
// outside the grid, sets no cell.
__device__ __forceinline__ void occupancy_mark(uint8_t* occupancy, double px0, double px1, int cell_size, int grid_n_cols, int grid_n_rows) {
  const double qc = px0 / (double)cell_size, qr = px1 / (double)cell_size;
  if (qc > -1.0 && qc < (double)grid_n_cols && qr > -1.0 && qr < (double)grid_n_rows) {  // (false for NaN)
    const int col = (int)qc, row = (int)qr;
    if (col >= 0 && col < grid_n_cols && row >= 0 && row < grid_n_rows) occupancy[(size_t)row * grid_n_cols + col] = 1;
  }
}

}  // namespace svo_dev
