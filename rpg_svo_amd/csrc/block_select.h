// block_select.h -- what the bootstrap kernels (K8 klt_track.hip, K9 homography_init.hip, K10 first_map.hip) do with a
// workgroup's list: compact it in index order, and take the value of one rank out of it.  Integer work apart from the
// comparisons of the rank count, so nothing here depends on the contraction mode of the including file.
#pragma once
#ifndef SVO_HOST_MATH_TEST  // (see device_math.h)
#include <hip/hip_runtime.h>
#endif

namespace svo_dev {

// One step of an order-preserving compaction over a workgroup of 64 * WAVES work-items (t = threadIdx.x): -> the slot of
// this work-item among the `on` ones, counted from m in index order (meaningful where `on` holds); m advances by the
// step's total.  __ballot + popcount inside a wave, the wave counts through s_wcnt[WAVES] in LDS.  Two barriers: call it
// from workgroup-uniform code.  The first barrier also keeps a step's s_wcnt from the reads of the step before.
template <int WAVES>
__device__ __forceinline__ int block_compact_step(bool on, int t, int* s_wcnt, int& m) {
  const unsigned long long mask = __ballot(on);
  const int lane = t & 63, w = t >> 6;
  __syncthreads();
  if (lane == 0) s_wcnt[w] = (int)__popcll(mask);
  __syncthreads();
  int before = m;
#pragma unroll
  for (int k = 0; k < WAVES; ++k) {
    before += k < w ? s_wcnt[k] : 0;
    m += s_wcnt[k];
  }
  return before + (int)__popcll(mask & ((1ull << lane) - 1ull));
}

// vk::getMedian's nth_element by counting: the value of rank k (from 0, ascending) among the v[j], j < n, with on(j),
// stored to *out by the one work-item (of THREADS, t = threadIdx.x) that holds it.  Equal values are ordered by index --
// they are the same value -- so exactly one participant has each rank.  v and whatever on() reads are in place before
// the call; the barrier before *out is read is the caller's, and so is the case of no participant or k beyond them
// (nothing is stored).  n * n compares per workgroup: for lists of about a thousand.
template <int THREADS, class On>
__device__ __forceinline__ void block_rank_select(const double* v, int n, int k, int t, On on, double* out) {
  for (int i = t; i < n; i += THREADS) {
    if (!on(i)) continue;
    const double x = v[i];
    int rank = 0;
    // (& and | on purpose: without branches the compiler unrolls the count, and drops a mask the comparisons imply, K10's)
    for (int j = 0; j < n; ++j) rank += (int)(bool(on(j)) & ((v[j] < x) | ((v[j] == x) & (j < i))));
    if (rank == k) *out = x;
  }
}

}  // namespace svo_dev
