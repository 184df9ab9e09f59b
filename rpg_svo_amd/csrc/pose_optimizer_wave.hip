// pose_optimizer_wave.hip -- K4 (default form): batched pose_optimizer::optimizeGaussNewton, one
// WAVE per frame, one frame per workgroup (PW_WAVES), no workgroup barrier.
//
// Replaces svo::pose_optimizer::optimizeGaussNewton (svo/src/pose_optimizer.cpp:28-161) to a
// stated tolerance (pose within 1e-9 of the reference, SE(3) log-map norm; pruning decisions on
// the residuals of that pose: e2 > thresh^2).  The bit-ordered variant that reproduces the
// reference's summation order (pose_optimizer.hip, svo_hip_pose_optimize_ordered) stays as the
// checker; this kernel is what the pipeline runs:
//
//   * a wave reads its row once, in two round trips to memory (the flag bytes of the whole row; then f, pos, level of the live
//     slots and the pose, all requested before the one wait), and writes the LIVE observations side by
//     side, in index order (position = ballot + popcount of the lanes below: nothing depends on timing), into its own block
//     of the workgroup's dynamic LDS: px py pz ux uy as f64, the level scale as f32, the slot it came from as u8 -- 45 bytes
//     per observation, structure of arrays over n_stride (rounded up to 8) positions, 9 000 bytes per wave (= workgroup) at
//     n_stride = 200, so that sixteen of them fit a CU's 160 KB, and a finished frame frees its block for the next workgroup at
//     once (11 520 bytes and fourteen at n_stride = 256).  Nothing is re-read from HBM between Gauss-Newton
//     iterations, and the observations cost no registers: 121 VGPRs, no scratch, four waves per SIMD (occupancy is what hides the f64
//     dependency chains of the solve: there is no memory access in the loop to overlap them with);
//   * an iteration walks the block in ceil(n_live / 64) trips -- a runtime loop, so a frame of 172 live observations in a
//     row of 200 pays three trips, not four; a lane past n_live in the last trip reads the last live record again and counts
//     with weight 0.  The two passes around the loop (MAD scale / initial median, pruning / final median) read the same block;
//     pruning clears has_point at the slot the record came from.  The flags and the pose are read from has_point_in / T_in
//     and written to has_point / T, which may be the same arrays (in place) or others (svo_hip_pose_optimize_into: the first
//     pass then carries every flag byte of the row and the pose over, so that nobody copies them beforehand).  The block is the wave's alone: same-wave DS operations
//     execute in order, SVO_WAVE_LDS_FENCE keeps the compiler from moving the reads above the stores, and there is no barrier;
//   * the 25 distinct non-zero f64 sums of an iteration (18 entries of A -- A(0,1) is identically zero, A(1,1) is A(0,0) and
//     A(1,4) is -A(0,3) bit for bit --, b[6], chi2) are accumulated per lane and reduced over the wave with a TRANSPOSING
//     butterfly (v_permlane32_swap / v_permlane16_swap / DPP): 32 f64 additions instead of
//     25 x 6, no LDS round trip, no ordered chain;
//   * the 6x6 solve, SE3::exp(dT)*T and the stop / rollback rules run redundantly in every lane
//     on wave-uniform values (readlane broadcasts): no serial lane, no barrier.  The solve is an
//     unpivoted LDL^T; only when a pivot collapses (rank-deficient systems of a handful of
//     observations) the wave falls back to Eigen's pivoted algorithm, as the ordered kernel uses;
//   * MAD scale and the two reported medians are exact order statistics found by a bitwise
//     radix select over the wave (ballot + popcount per bit), not by O(n^2) rank counting; its keys (up to four per lane)
//     stay in registers.
// The argument block, the row limits, the Tukey weight, the codes of `ran` and the result lines are the ordered kernel's too:
// pose_common.h.
#include "pose_common.h"
#include "track_math.h"
#include "wave_reduce.h"

using namespace svo_capi;
using namespace svo_dev;

namespace {

using namespace svo_track;

// Frames (= waves) per workgroup: ONE.  Nothing ties the waves of a workgroup together but the LDS, which the hardware hands
// out per workgroup and takes back only when its LAST wave ends: with four frames per workgroup a frame that rolled back after
// two iterations held its block until the slowest of its three neighbours was through (on the benchmark's rows E[max of 4] /
// E[T] = 1.54 in iterations), and no new workgroup could start in its place.  The launch bounds, the block offset, the grid and
// the byte count of the launch follow this one number; 2 and 4 were the other two builds of
// profiles/r08a_k4_one_frame_per_workgroup.txt (compose + K4 0.2170 ms at 4, 0.2079 at 2, 0.2002 at 1; the same bytes out).
constexpr int PW_WAVES = 1;
constexpr int PW_TRIPS = POSE_WAVE_MAX_STRIDE / 64;  // trips of 64 slots a row can have
constexpr int PW_MINW = 4;  // waves per SIMD asked of the register allocator (<= 128 VGPRs)

// The pose (R, t, quaternion, rollback copy) is 38 doubles: kept in VGPRs it would cost 76 registers per lane next to
// the resident observations; uniform_f64 (device_math.h) moves them to SGPRs.
__device__ __forceinline__ void uni_se3(Se3& T) {
#pragma unroll
  for (int k = 0; k < 4; ++k) T.q[k] = uniform_f64(T.q[k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) T.t[k] = uniform_f64(T.t[k]);
}


// Sums v[0..31] over the 64 lanes.  On return lanes 2j and 2j+1 hold the wave total of v[j].
__device__ __forceinline__ double wave_reduce32_f64(const double v[32], int lane) {
  double r[16], q[8], t[4], u[2];
#pragma unroll
  for (int k = 0; k < 16; ++k) r[k] = swap32_add(v[k], v[k + 16]);
#pragma unroll
  for (int k = 0; k < 8; ++k) q[k] = swap16_add(r[k], r[k + 8]);
  {
    const bool hi = (lane & 8) != 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double mine = hi ? q[k + 4] : q[k], send = hi ? q[k] : q[k + 4];
      t[k] = mine + dpp_f64<DPP_ROW_ROR8>(send);
    }
  }
  {
    const bool hi = (lane & 4) != 0;  // partner 7-i inside each 8 lanes has the other bit 2
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double mine = hi ? t[k + 2] : t[k], send = hi ? t[k] : t[k + 2];
      u[k] = mine + dpp_f64<DPP_ROW_HALF_MIRROR>(send);
    }
  }
  const bool hi = (lane & 2) != 0;
  const double mine = hi ? u[1] : u[0], send = hi ? u[0] : u[1];
  double w = mine + dpp_f64<DPP_QUAD_XOR2>(send);
  w += dpp_f64<DPP_QUAD_XOR1>(w);
  return w;
}

// sqrt for x >= 0 (v_rsq_f64 seed + two coupled Newton steps), 0 for x == 0
__device__ __forceinline__ double fast_sqrt(double x) {
  const double r = __builtin_amdgcn_rsq(x);
  double g = x * r;
  const double h = 0.5 * r;
  g = fma(fma(-g, g, x), h, g);
  g = fma(fma(-g, g, x), h, g);
  return fmax(g, 0.0);  // x == 0: rsq is +inf and g a NaN, which the maximum drops (one v_max_f64 for a compare and two selects)
}

// ldlt6_factor (device_math.h) with the six pivot reciprocals by v_rcp_f64 + Newton.  A vanished pivot leaves LD[15 + j] = 0
// and a column that means nothing (v * 0: ldlt6_factor keeps v): the only caller hands such a frame to the ordered kernel
// (pivots_ok) before anything reads the factor -- fifteen selects per Gauss-Newton iteration less.
// (Skipping the fourth observation slot of a frame of <= 192 observations behind a scalar branch, with the observations in
// registers: five more 8-byte spills, 0.232 -> 0.235 ms, profiles/r06ag_*.  With the observations in LDS the trips are a
// runtime loop and the fourth one is simply not made.)
__device__ __forceinline__ void ldlt6_factor_fast(const double H[21], double LD[21]) {
  double d[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double dj = H[sym6(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) dj -= LD[low6(j, k)] * LD[low6(j, k)] * d[k];
    d[j] = dj;
    const bool ok = fabs(dj) > 2.2250738585072014e-308;
    const double inv = ok ? fast_rcp(dj) : 0.0;
    LD[15 + j] = inv;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = H[sym6(j, i)];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= LD[low6(i, k)] * LD[low6(j, k)] * d[k];
      LD[low6(i, j)] = v * inv;
    }
  }
}

// Sophus SE3::exp (device_math.h se3_exp) with one reciprocal instead of three divisions
__device__ __forceinline__ void se3_exp_fast(const double xi[6], double q[4], double t[3]) {
  const double ox = xi[3], oy = xi[4], oz = xi[5];
  const double theta_sq = ox * ox + oy * oy + oz * oz;
  const double theta = fast_sqrt(theta_sq);
  double s_h, c_h;
  sincos_small(0.5 * theta, &s_h, &c_h);
  const double ux = xi[0], uy = xi[1], uz = xi[2];
  if (theta < 1e-10) {
    const double theta_po4 = theta_sq * theta_sq;
    const double imag_factor = 0.5 - 0.0208333 * theta_sq + 0.000260417 * theta_po4;
    q[0] = c_h; q[1] = imag_factor * ox; q[2] = imag_factor * oy; q[3] = imag_factor * oz;
    quat_rot(q, xi, t);
  } else {
    const double it = fast_rcp(theta);
    const double imag_factor = s_h * it;
    q[0] = c_h; q[1] = imag_factor * ox; q[2] = imag_factor * oy; q[3] = imag_factor * oz;
    const double it2 = it * it;
    const double s_t = 2.0 * s_h * c_h;
    const double c1 = (2.0 * s_h * s_h) * it2;
    const double c2 = (theta - s_t) * (it2 * it);
    const double wx = oy * uz - oz * uy, wy = oz * ux - ox * uz, wz = ox * uy - oy * ux;
    const double wwx = oy * wz - oz * wy, wwy = oz * wx - ox * wz, wwz = ox * wy - oy * wx;
    t[0] = ux + c1 * wx + c2 * wwx;
    t[1] = uy + c1 * wy + c2 * wwy;
    t[2] = uz + c1 * wz + c2 * wwz;
  }
}

// Sophus SE3::operator* with the renormalisation by v_rsq_f64 + Newton
__device__ __forceinline__ Se3 se3_compose_fast(const Se3& a, const Se3& b) {
  Se3 r;
  double rt[3];
  quat_rot(a.q, b.t, rt);
  r.t[0] = a.t[0] + rt[0]; r.t[1] = a.t[1] + rt[1]; r.t[2] = a.t[2] + rt[2];
  quat_mul(a.q, b.q, r.q);
  quat_normalize_fast(r.q);
  return r;
}

// Exact order statistic: the value of rank k (0-based) among the wave's NPL*64 keys.  Keys are
// bit patterns of non-negative floats/doubles (order-isomorphic to unsigned integers);
// non-participants hold +inf.  One ballot + popcount per key and bit; the walk down the bits ends as
// soon as the interval [prefix, prefix + 2^(bit+1)) holds a single key, which is then fetched from
// its owner lane (distinct values: ~20 of the 31 / 63 steps).
template <int NPL, typename K>
__device__ __forceinline__ K radix_select(const K key[NPL], int k, int top_bit) {
  K prefix = 0;
  int cnt_lo = 0, cnt_hi = NPL * 64;  // #keys < prefix, #keys < prefix + 2^(bit+1)
  for (int bit = top_bit; bit >= 0; --bit) {
    const K cand = prefix | ((K)1 << bit);
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < NPL; ++j) cnt += __popcll(__ballot(key[j] < cand));  // (64-bit keys compared as doubles instead: no difference, profiles/r06al_*)
    if (cnt <= k) {
      prefix = cand;
      cnt_lo = cnt;
    } else {
      cnt_hi = cnt;
    }
    if (cnt_hi - cnt_lo == 1 && bit > 0) {
      const K upper = prefix + ((K)1 << bit);  // exclusive; bit is the width still undecided
      K found = prefix;
#pragma unroll
      for (int j = 0; j < NPL; ++j) {
        const unsigned long long m = __ballot(key[j] >= prefix && key[j] < upper);
        if (m) {
          const int src = __ffsll((long long)m) - 1;
          if (sizeof(K) == 8) {
            const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)key[j], src);
            const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)key[j] >> 32), src);
            found = (K)(((unsigned long long)hi << 32) | lo);
          } else {
            found = (K)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)key[j], src);
          }
        }
      }
      return found;
    }
  }
  return prefix;
}

// every pivot of the unpivoted LDL^T (LD[15+k] = 1/d_k, 0 where d_k vanished) above 1e-9 of the
// largest diagonal entry
__device__ __forceinline__ bool pivots_ok(const double A[21], const double LD[21]) {
  double dmax = 0.0, imax = 0.0;
  bool zero = false;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    dmax = fmax(dmax, fabs(A[sym6(k, k)]));
    const double id = fabs(LD[15 + k]);
    zero = zero || !(id > 0.0);
    imax = fmax(imax, id);
  }
  // d_min = 1/imax > 1e-9 * dmax
  return !zero && (imax * dmax * 1e-9 < 1.0);
}

// broadcast of a runtime-indexed pair of lanes is not needed: indices are compile-time
template <int J>
__device__ __forceinline__ double bcast(double v) { return readlane_f64<2 * J>(v); }

// One observation as the passes read it back from the wave's LDS block
struct PwObs {
  double px, py, pz, ux, uy, k;
};

// The wave's private block of the workgroup's dynamic LDS, structure of arrays over `cap` positions (cap = n_stride rounded up
// to 8, so that every array starts 8-byte aligned): px py pz ux uy as f64, the level scale as f32, the original slot as u8 --
// 45 bytes per position.
struct PwBlock {
  double* d;      // [5][cap]
  float* k;       // [cap]
  uint8_t* slot;  // [cap]
  int cap;
  __device__ __forceinline__ PwObs load(int c) const {  // c: clamped by the caller
    PwObs o;
    o.px = d[c]; o.py = d[cap + c]; o.pz = d[2 * cap + c]; o.ux = d[3 * cap + c]; o.uy = d[4 * cap + c];
    o.k = (double)k[c];
    return o;
  }
};
constexpr int PW_BYTES_PER_OBS = 5 * 8 + 4 + 1;

// e = (u - project2d(T p)) * sqrt_inv_cov of one observation, e2 = |e|^2, and what the Jacobian is formed from: 1/z and the
// normalised coordinates of T p.  The two median passes read e2, the Gauss-Newton loop everything: the same residuals.
struct PwRes {
  double zi, xn, yn, e0, e1, e2;
};
__device__ __forceinline__ PwRes pw_residual(const PwObs& o, const double R[9], const double t[3]) {
  const double x = R[0] * o.px + R[1] * o.py + R[2] * o.pz + t[0];
  const double y = R[3] * o.px + R[4] * o.py + R[5] * o.pz + t[1];
  const double z = R[6] * o.px + R[7] * o.py + R[8] * o.pz + t[2];
  PwRes r;
  r.zi = fast_rcp(z);
  r.xn = x * r.zi;
  r.yn = y * r.zi;
  r.e0 = (o.ux - r.xn) * o.k;  // e *= sqrt_inv_cov
  r.e1 = (o.uy - r.yn) * o.k;
  r.e2 = r.e0 * r.e0 + r.e1 * r.e1;
  return r;
}

// rank k among the keys of the first `trips` (wave-uniform, 1..PW_TRIPS) of kd
__device__ __forceinline__ double pw_select(const unsigned long long kd[PW_TRIPS], int trips, int k) {
  static_assert(PW_TRIPS == 4, "the chain below names every number of trips");
  unsigned long long r;
  if (trips <= 1) r = radix_select<1, unsigned long long>(kd, k, 62);
  else if (trips == 2) r = radix_select<2, unsigned long long>(kd, k, 62);
  else if (trips == 3) r = radix_select<3, unsigned long long>(kd, k, 62);
  else r = radix_select<4, unsigned long long>(kd, k, 62);
  return __longlong_as_double((long long)r);
}

// Every load (and store) this wave has issued so far is through: ONE wait where the compiler would place one per use, and
// a line no load moves across.  s_waitcnt vmcnt(0) alone: expcnt 7 and lgkmcnt 15 are "do not wait" (gfx9 encoding: vmcnt in
// bits 3:0 and 15:14, expcnt in 6:4, lgkmcnt in 11:8).  The host emulation runs its loads one after the other anyway.
__device__ __forceinline__ void pw_loads_done() {
#ifdef __HIP_DEVICE_COMPILE__
  __builtin_amdgcn_s_waitcnt(0x0F70);
#endif
}

// The 25 sums in reduction order (two more of the 27 non-zero entries are copies: A(1,1) is the expression of A(0,0), since
// j11 == j00, and A(1,4) is -A(0,3) bit for bit, since j14 == -j03 and rounding to nearest is symmetric):
//   0..4   A(0,0) A(0,2) A(0,3) A(0,4) A(0,5)
//   6,7,9  A(1,2) A(1,3) A(1,5)          (5 and 8 stay zero)
//   10..19 A(2,2) A(2,3) A(2,4) A(2,5) A(3,3) A(3,4) A(3,5) A(4,4) A(4,5) A(5,5)
//   20..25 b[0..5]   26 chi2
__global__ void __launch_bounds__(64 * PW_WAVES, PW_MINW) pose_opt_wave_kernel(const PoseArgs a) {
  SVO_DYNAMIC_LDS(double, pw_dyn);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int b = __builtin_amdgcn_readfirstlane(blockIdx.x * PW_WAVES + wave);  // (the wave's: addresses off it stay in SGPRs)
  if (b >= a.B) return;
  const int n = pose_row_n(a, __builtin_amdgcn_readfirstlane(a.n[b]));
  const size_t base = (size_t)b * a.n_stride;
  const double focal = fabs(a.cam.fx);

  // ---- this wave's observations: the live ones, in index order, side by side in LDS for the whole call -----------
  PwBlock blk;
  blk.cap = pose_cap(a.n_stride);
  blk.d = pw_dyn + (size_t)wave * (blk.cap / 8) * PW_BYTES_PER_OBS;  // (cap * 45 bytes per wave: a multiple of 8)
  blk.k = reinterpret_cast<float*>(blk.d + 5 * blk.cap);
  blk.slot = reinterpret_cast<uint8_t*>(blk.k + blk.cap);
  // Not in place (svo_hip_pose_optimize_into): this pass reads every flag of the frame anyway, so it also carries the row over to
  // the output -- all n_stride slots, those beyond n as they came in -- and every exit below leaves a pose in a.T.
  const bool carry = a.has_point_in != a.has_point;
  // Two round trips to memory for the whole row, not two per trip of 64 slots: every load below is unconditional (an index
  // outside the frame is moved into the row and the answer dropped afterwards) and waited for once, by pw_loads_done, because a
  // load that only a branch uses is moved into that branch and waited for there.  First the flag bytes of all PW_TRIPS trips ...
  uint8_t flag[PW_TRIPS];
#pragma unroll
  for (int j = 0; j < PW_TRIPS; ++j) {
    const int i = j * 64 + lane;
    flag[j] = a.has_point_in[base + (i < a.n_stride ? i : a.n_stride - 1)];
  }
  pw_loads_done();
  // ... then who is live and where it goes: position = the number of live observations before this one (ballot + popcount of
  // the lanes below: nothing depends on timing); < n <= cap by construction, clamped all the same ...
  bool live[PW_TRIPS];
  int at[PW_TRIPS];
  int n_live = 0;
#pragma unroll
  for (int j = 0; j < PW_TRIPS; ++j) {
    live[j] = (j * 64 + lane < n) && flag[j] != 0;
    const unsigned long long m = __ballot(live[j]);
    const int c = n_live + __popcll(m & ((1ull << lane) - 1ull));
    at[j] = c < blk.cap ? c : blk.cap - 1;
    n_live += __popcll(m);
  }
  // ... then pos, f and level of all trips (a slot that is not live asks for slot 0 of the row: one address for all such lanes) ...
  double p[PW_TRIPS][3], f[PW_TRIPS][3];
  int lv[PW_TRIPS];
#pragma unroll
  for (int j = 0; j < PW_TRIPS; ++j) {
    const size_t src = base + (live[j] ? j * 64 + lane : 0);
#pragma unroll
    for (int k = 0; k < 3; ++k) p[j][k] = a.pos[3 * src + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) f[j][k] = a.f[3 * src + k];
    lv[j] = a.level[src];
  }
  const double t_raw = a.T_in[12 * b + (lane < 12 ? lane : 11)];  // and the pose, one of its twelve doubles per lane
  pw_loads_done();
  // Not in place: the pose goes to the output as it came in, here and once -- the exits that leave it alone (nothing live, a
  // frame handed over) find it done, so that whoever works on the outputs next (the ordered kernel, the caller) finds the
  // frame, and the last line of the Gauss-Newton loop writes over it.
  if (a.T_in != a.T && lane < 12) a.T[12 * b + lane] = t_raw;
  if (carry) {  // (and the flags, behind the second wait: no load waits for these stores)
#pragma unroll
    for (int j = 0; j < PW_TRIPS; ++j) {
      const int i = j * 64 + lane;
      if (i < a.n_stride) a.has_point[base + i] = flag[j];
    }
  }
  // ... and the records into LDS, trip after trip.
#pragma unroll
  for (int j = 0; j < PW_TRIPS; ++j) {
    if (live[j]) {
      const int c = at[j];
      blk.d[c] = p[j][0]; blk.d[blk.cap + c] = p[j][1]; blk.d[2 * blk.cap + c] = p[j][2];
      blk.d[3 * blk.cap + c] = f[j][0] / f[j][2];  // vk::project2d(f), once
      blk.d[4 * blk.cap + c] = f[j][1] / f[j][2];
      blk.k[c] = pow2_inv_f32(lv[j]);  // == 1.0f / (float)(1 << level), from exponent bits
      blk.slot[c] = (uint8_t)(j * 64 + lane);
    }
  }
  if (n_live == 0) {  // errors.empty(): return before touching anything (:57-58)
    if (lane == 0) a.ran[b] = POSE_RAN_NONE;
    return;
  }
  SVO_WAVE_LDS_FENCE();  // the block is this wave's alone: its DS operations execute in order, no barrier
  // Trip t gives lane l the observation at position 64 t + l.  A lane past n_live in the last trip reads the last live
  // record again (a valid address and finite numbers) and counts with weight 0 / key +inf: the neutral record.
  const int last_pos = (n_live < blk.cap ? n_live : blk.cap) - 1;
  const int trips = (n_live + 63) >> 6;

  // model, wave-uniform (lanes 0 .. 11 hold the twelve doubles)
  Se3 T, T_old;
  {
    const double Rt[12] = {readlane_f64<0>(t_raw), readlane_f64<1>(t_raw), readlane_f64<2>(t_raw),  readlane_f64<3>(t_raw),
                           readlane_f64<4>(t_raw), readlane_f64<5>(t_raw), readlane_f64<6>(t_raw),  readlane_f64<7>(t_raw),
                           readlane_f64<8>(t_raw), readlane_f64<9>(t_raw), readlane_f64<10>(t_raw), readlane_f64<11>(t_raw)};
    se3_from_Rt(Rt, T);
  }
  uni_se3(T);
  T_old = T;
  double R[9];
  quat_to_R(T.q, R);
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = uniform_f64(R[k]);

  // ---- error scale (:45-60) and the median of chi2_vec_init (same residuals as iteration 0) ----
  // (This key loop and the one of the pruning pass below stay written out: as one function over the block, with the pruning
  // tail as a callable or handing e2 and `live` back per trip, the compiler commuted the operands of four v_fma_f64 of the
  // residual -- the same values, not the same instruction sequence; profiles/r13a_*.)
  double estimated_scale, med_init;
  {
    unsigned long long kd[PW_TRIPS];
#pragma unroll
    for (int j = 0; j < PW_TRIPS; ++j) {
      kd[j] = 0x7ff0000000000000ull;
      if (j < trips) {
        const int at = j * 64 + lane;
        const double e2 = pw_residual(blk.load(at < last_pos ? at : last_pos), R, T.t).e2;
        if (at < n_live) kd[j] = (unsigned long long)__double_as_longlong(e2);
      }
    }
    med_init = pw_select(kd, trips, n_live / 2);
    // The scale estimator's median is over errors = (float)sqrt(e2) of the same observations (:52-56), rank n / 2 as well:
    // sqrt and the conversion are monotone, so the rank-k error IS the image of the rank-k e2 -- one selection, not two
    // (equal images of different e2 are the same value).
    const float median_f = (float)sqrt(med_init);
    estimated_scale = (double)(POSE_MAD_NORMALISER * median_f);  // MADScaleEstimator::compute
  }

  // ---- Gauss-Newton (:66-121) ----------------------------------------------------------
  double scale = estimated_scale;
  double chi2 = 0.0;
  if (a.n_iter == 0) {  // Cov_ of a never-formed A: the ordered kernel reproduces what the reference leaves behind
    if (lane == 0) a.ran[b] = POSE_RAN_ORDERED;
    return;
  }
  for (int iter = 0; iter < a.n_iter; ++iter) {
    if (iter == 5) scale = 0.85 / focal;
    const double inv_scale = 1.0 / scale;
    double A[21];  // packed upper triangle of this iteration's normal matrix (sym6 order)
    double acc[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (int j = 0; j < trips; ++j) {  // a lane adds its observations in trip order
      const int at = j * 64 + lane;
      const PwObs o = blk.load(at < last_pos ? at : last_pos);
      const PwRes r = pw_residual(o, R, T.t);
      const double zi = r.zi, xn = r.xn, yn = r.yn, k = o.k, e0 = r.e0, e1 = r.e1, e2 = r.e2;
      const float wf = pose_tukey_weight((float)(fast_sqrt(e2) * inv_scale));
      const double w = at < n_live ? (double)wf : 0.0;
      // Frame::jacobian_xyz2uv (frame.h:116-138), rows J0 / J1 scaled by sqrt_inv_cov; j11 == j00, j14 == -j03
      const double j00 = -zi * k, j02 = xn * zi * k, j03 = xn * yn * k, j04 = -(1.0 + xn * xn) * k, j05 = yn * k;
      const double j12 = yn * zi * k, j13 = (1.0 + yn * yn) * k, j14 = -j03, j15 = -xn * k;
      const double w00 = w * j00, w02 = w * j02, w03 = w * j03, w04 = w * j04, w05 = w * j05;
      const double w11 = w00, w12 = w * j12, w13 = w * j13, w14 = w * j14, w15 = w * j15;
      acc[0] = fma(w00, j00, acc[0]);
      acc[1] = fma(w00, j02, acc[1]);
      acc[2] = fma(w00, j03, acc[2]);
      acc[3] = fma(w00, j04, acc[3]);
      acc[4] = fma(w00, j05, acc[4]);
      acc[6] = fma(w11, j12, acc[6]);
      acc[7] = fma(w11, j13, acc[7]);
      acc[9] = fma(w11, j15, acc[9]);
      acc[10] = fma(w02, j02, fma(w12, j12, acc[10]));
      acc[11] = fma(w02, j03, fma(w12, j13, acc[11]));
      acc[12] = fma(w02, j04, fma(w12, j14, acc[12]));
      acc[13] = fma(w02, j05, fma(w12, j15, acc[13]));
      acc[14] = fma(w03, j03, fma(w13, j13, acc[14]));
      acc[15] = fma(w03, j04, fma(w13, j14, acc[15]));
      acc[16] = fma(w03, j05, fma(w13, j15, acc[16]));
      acc[17] = fma(w04, j04, fma(w14, j14, acc[17]));
      acc[18] = fma(w04, j05, fma(w14, j15, acc[18]));
      acc[19] = fma(w05, j05, fma(w15, j15, acc[19]));
      // b -= J' e w
      acc[20] = fma(-w00, e0, acc[20]);
      acc[21] = fma(-w11, e1, acc[21]);
      acc[22] = fma(-w02, e0, fma(-w12, e1, acc[22]));
      acc[23] = fma(-w03, e0, fma(-w13, e1, acc[23]));
      acc[24] = fma(-w04, e0, fma(-w14, e1, acc[24]));
      acc[25] = fma(-w05, e0, fma(-w15, e1, acc[25]));
      acc[26] = fma(e2, w, acc[26]);
    }
    const double tot = wave_reduce32_f64(acc, lane);
    const double s0 = bcast<0>(tot), s1 = bcast<1>(tot), s2 = bcast<2>(tot), s3 = bcast<3>(tot), s4 = bcast<4>(tot);
    const double s6 = bcast<6>(tot), s7 = bcast<7>(tot), s9 = bcast<9>(tot);
    const double s10 = bcast<10>(tot), s11 = bcast<11>(tot), s12 = bcast<12>(tot), s13 = bcast<13>(tot);
    const double s14 = bcast<14>(tot), s15 = bcast<15>(tot), s16 = bcast<16>(tot), s17 = bcast<17>(tot);
    const double s18 = bcast<18>(tot), s19 = bcast<19>(tot);
    const double bv[6] = {bcast<20>(tot), bcast<21>(tot), bcast<22>(tot), bcast<23>(tot), bcast<24>(tot), bcast<25>(tot)};
    const double new_chi2 = bcast<26>(tot);
    A[sym6(0, 0)] = s0; A[sym6(0, 1)] = 0.0; A[sym6(0, 2)] = s1; A[sym6(0, 3)] = s2; A[sym6(0, 4)] = s3; A[sym6(0, 5)] = s4;
    A[sym6(1, 1)] = s0; A[sym6(1, 2)] = s6; A[sym6(1, 3)] = s7; A[sym6(1, 4)] = -s2; A[sym6(1, 5)] = s9;
    A[sym6(2, 2)] = s10; A[sym6(2, 3)] = s11; A[sym6(2, 4)] = s12; A[sym6(2, 5)] = s13;
    A[sym6(3, 3)] = s14; A[sym6(3, 4)] = s15; A[sym6(3, 5)] = s16;
    A[sym6(4, 4)] = s17; A[sym6(4, 5)] = s18; A[sym6(5, 5)] = s19;

    // dT = A.ldlt().solve(b) (:97).  Unpivoted LDL^T (stable for the SPD normal equations).  A
    // collapsed pivot means a (nearly) rank-deficient system -- fewer observations than degrees
    // of freedom -- where the reference's answer is decided by the rounding of its own ordered
    // sums inside Eigen's pivoted algorithm: such a frame is handed to the ordered kernel
    // untouched (ran = POSE_RAN_ORDERED; the outputs hold the frame's flags and pose as they came in and nothing else has been written).
    double dT[6];
    double LD[21];
    ldlt6_factor_fast(A, LD);
    if (!pivots_ok(A, LD)) {
      if (lane == 0) a.ran[b] = POSE_RAN_ORDERED;
      return;
    }
    ldlt6_solve(LD, bv, dT);

    bool last = false;
    if ((iter > 0 && new_chi2 > chi2) || isnan(dT[0])) {  // check if error increased (:100-107)
      T = T_old;  // roll-back
      last = true;
    } else {
      // update the model: T_new = SE3::exp(dT) * T  (:110)
      Se3 ex;
      se3_exp_fast(dT, ex.q, ex.t);
      T_old = T;
      T = se3_compose_fast(ex, T);
      uni_se3(T);
      chi2 = new_chi2;
      double nm = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) nm = fmax(nm, fabs(dT[k]));
      last = nm <= SVO_EPS;  // stop when converged (:120)
    }
    quat_to_R(T.q, R);
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = uniform_f64(R[k]);
    last = last || iter + 1 == a.n_iter;
    if (last) {
      // covariance (:124-126): (A f^2)^-1 = A^-1 / f^2 with the A of the last evaluated iteration,
      // from the factor that is still in registers; lane j (< 6) solves for column j
      if (a.Cov) {
        double e[6], x[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) e[i] = (i == lane) ? 1.0 : 0.0;
        ldlt6_solve(LD, e, x);
        const double if2 = 1.0 / (focal * focal);
        if (lane < 6) {
#pragma unroll
          for (int i = 0; i < 6; ++i) a.Cov[36 * b + i * 6 + lane] = x[i] * if2;
        }
      }
      break;
    }
  }
  if (lane == 0) se3_to_Rt(T, a.T + 12 * b);

  // ---- prune outliers (:128-145) and the median of chi2_vec_final ---------------------------
  const double reproj_thresh_scaled = a.reproj_thresh / focal;
  const double reproj_thresh2 = reproj_thresh_scaled * reproj_thresh_scaled;
  int n_deleted = 0;
  double med_final;
  {
    unsigned long long kd[PW_TRIPS];
#pragma unroll
    for (int j = 0; j < PW_TRIPS; ++j) {
      kd[j] = 0x7ff0000000000000ull;
      if (j < trips) {
        const int at = j * 64 + lane;
        const int c = at < last_pos ? at : last_pos;
        const double e2 = pw_residual(blk.load(c), R, T.t).e2;
        const bool live = at < n_live;
        if (live) kd[j] = (unsigned long long)__double_as_longlong(e2);
        // e.norm() > reproj_thresh_scaled (:136) as e2 > thresh^2: the pose this kernel arrives at differs from the reference's
        // by up to 1e-9, which moves e2 by far more than the rounding of a division or a square root -- no decision hangs on them
        const bool prune = live && e2 > reproj_thresh2;
        if (prune) {
          const int slot = blk.slot[c];  // where the observation came from (< n: only such slots were stored)
          if (slot < n) a.has_point[base + slot] = 0;  // (*it)->point = NULL
        }
        n_deleted += __popcll(__ballot(prune));
      }
    }
    med_final = pw_select(kd, trips, n_live / 2);
  }
  if (lane == 0) pose_write_result(a, b, focal, estimated_scale, med_init, med_final, n_live, n_deleted);
}

}  // namespace

namespace svo_track {

// n_stride <= POSE_WAVE_MAX_STRIDE only (the radix select keeps PW_TRIPS keys per lane in registers); the caller falls back to
// the ordered kernel beyond
int launch_pose_wave(const PoseArgs& a, hipStream_t s) {
  const int grid = (a.B + PW_WAVES - 1) / PW_WAVES;
  const size_t lds = (size_t)PW_WAVES * pose_cap(a.n_stride) * PW_BYTES_PER_OBS;  // <= PW_WAVES * 11 520 bytes
  hipLaunchKernelGGL(pose_opt_wave_kernel, dim3(grid), dim3(64 * PW_WAVES), lds, s, a);
  return check_launch();
}

}  // namespace svo_track
