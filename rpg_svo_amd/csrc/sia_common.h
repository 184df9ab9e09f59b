// sia_common.h -- pieces shared by the two K1 kernels (sparse_align.hip: one workgroup of several waves per
// problem; sparse_align_wave.hip: one wave per problem): the argument block, the unaligned row loads of the
// 8-bit pyramid levels and the window-cache cuts.
#pragma once
#include "capi_common.h"
#include "device_math.h"
#include "track_math.h"
#include "wave_reduce.h"

namespace svo_sia {

using namespace svo_capi;
using namespace svo_dev;

struct SiaArgs {
  svo_hip_pyr_layout L;
  const uint8_t* store;
  const int32_t* ref_slot;
  const int32_t* cur_slot;
  const int32_t* n;
  int n_stride;
  const double* px;
  const double* xyz;
  const uint8_t* valid;
  svo_hip_sia_params P;
  const double* T_in;
  double* T_out;
  double* H_out;
  int32_t* n_tracked;
  int32_t* iters;
  double* chi2;
  int32_t* status;
  // A frame split over several workgroups (sparse_align.hip, PARTS > 1): the number of frames (the grid is padded), the
  // exchange blocks (one SIA_X_BLOCK-chunk block per frame).  NULL / 0 otherwise.
  int B = 0;
  void* xw = nullptr;
};

// ---- the exchange between the workgroups of a split frame -------------------------------------------------------------
// One 16-byte chunk = a partial sum and the epoch of the exchange it belongs to, written and read as ONE access: data and
// flag arrive together, no counter, no atomic, no fence.  PLACEMENT-INDEPENDENT: a part stores its chunks write-through
// (sc1: the line leaves the XCD's L2 for memory) and every wave polls the other parts' chunks with sc1 loads (which miss
// the polling CU's vector L1 and are served below it) until they carry this exchange's epoch -- the agent-scope forms,
// correct wherever the dispatcher puts the four workgroups (it promises nothing; ids 8 apart usually share an XCD, which
// is a matter of speed only).  Round 6 first built this with sc0 stores kept in a shared L2: it never saw its siblings
// inside the real kernel although a microbenchmark of the same instructions did (profiles/r06f_*): placement is not a
// contract.  Each 8-byte half of a chunk carries the epoch, so that a reader can tell a torn 16-byte read (never
// observed on gfx950) from a whole one.  Epochs never repeat in a block: a frame's block ends with a word holding the last
// epoch used in it (zero when the block is new), every part reads it when it starts and part 0 writes it back when the
// frame is done, so a launch continues counting where the block's last user stopped and no chunk an earlier launch (or an
// earlier replay of a captured one) left behind can carry an epoch this launch waits for -- nothing is cleared per launch.
struct XChunk {
  unsigned lo, tag0, hi, tag1;
};
static_assert(sizeof(XChunk) == 16, "one 16-byte access");
constexpr int SIA_X_SLOTS = 16;   // chunks per part and buffer half of the per-iteration exchange (9 used: 8 sums + "changed")
constexpr int SIA_XH_SLOTS = 24;  // ... of the H exchange (21 used)
constexpr int SIA_X_MAX_PARTS = 4;
constexpr int SIA_X_CHUNKS = 2 * SIA_X_MAX_PARTS * (SIA_X_SLOTS + SIA_XH_SLOTS);  // exchange chunks per frame ...
constexpr int SIA_X_BLOCK = SIA_X_CHUNKS + 1;                                     // ... + the chunk that holds the block's last epoch

#ifndef SVO_HOST_MATH_TEST
__device__ __forceinline__ void sia_xstore(XChunk* p, double v, unsigned epoch) {
  typedef unsigned int u4 __attribute__((ext_vector_type(4)));
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  u4 w;
  w.x = (unsigned)b; w.y = epoch; w.z = (unsigned)(b >> 32); w.w = epoch;
  // The wait states behind the store are part of it: a VMEM store of more than 8 bytes reads its data registers for a few
  // cycles after issue, and the compiler's hazard recogniser does not look inside an asm statement -- it placed a VALU
  // write to the first data register pair right behind this store, and the quad of lanes the store had not read yet
  // (lanes 12-15 of 21) sent a chunk with a clobbered epoch that no reader ever accepted (profiles/r06h_*).
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 3" ::"v"(p), "v"(w) : "memory");
}
__device__ __forceinline__ XChunk sia_xload(const XChunk* p) {
  typedef unsigned int u4 __attribute__((ext_vector_type(4)));
  u4 w;
  asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(w) : "v"(p) : "memory");
  XChunk c;
  c.lo = w.x; c.tag0 = w.y; c.hi = w.z; c.tag1 = w.w;
  return c;
}
// the word at the end of a frame's block: the last epoch used in it
__device__ __forceinline__ void sia_xstore_epoch(XChunk* p, unsigned epoch) {
  typedef unsigned int u4 __attribute__((ext_vector_type(4)));
  u4 w;
  w.x = epoch; w.y = 0u; w.z = 0u; w.w = 0u;
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 3" ::"v"(p), "v"(w) : "memory");
}
// the value of chunk p once both its halves carry `epoch`; NaN (and failed = 1) when they never do: a part that is not
// running (the launcher only splits grids that are resident at once) must not hang the device
__device__ __forceinline__ double sia_xpoll(const XChunk* p, unsigned epoch, int& failed) {
  XChunk c = sia_xload(p);
  unsigned spins = 0;
  while (c.tag0 != epoch || c.tag1 != epoch) {
    if (++spins > (1u << 16)) {
      failed = 1;
      return __longlong_as_double(0x7ff8000000000000ll);
    }
    __builtin_amdgcn_s_sleep(1);
    c = sia_xload(p);
  }
  return __longlong_as_double((long long)(((unsigned long long)c.hi << 32) | c.lo));
}
#endif

using svo_pyr::load_window12;
using svo_pyr::run_start;

// Window rows are fetched as 12-byte runs of three aligned dwords (pyr_addr.h: run_start, load_run12, load_window12)
// and cut to the bytes wanted in registers.

// bytes [bo, bo+6] (bo in 0..5) of three consecutive dwords as floats
__device__ __forceinline__ void cut_row7(const uint32_t d[3], uint32_t bo, float out[7]) {
  const bool up = bo >= 4u;
  const uint32_t a = up ? d[1] : d[0], b = up ? d[2] : d[1], c = up ? 0u : d[2];
  const uint32_t sel = bo & 3u;
  const uint32_t lo = __builtin_amdgcn_alignbyte(b, a, sel);  // bytes 0..3
  const uint32_t hi = __builtin_amdgcn_alignbyte(c, b, sel);  // bytes 4..7
  out[0] = (float)(lo & 0xffu);
  out[1] = (float)((lo >> 8) & 0xffu);
  out[2] = (float)((lo >> 16) & 0xffu);
  out[3] = (float)(lo >> 24);
  out[4] = (float)(hi & 0xffu);
  out[5] = (float)((hi >> 8) & 0xffu);
  out[6] = (float)((hi >> 16) & 0xffu);
}

// bytes [bo, bo+4] (bo in 0..7) of three consecutive dwords as floats (the kernels without a window cache)
__device__ __forceinline__ void cut_row5_plain(const uint32_t d[3], uint32_t bo, float out[5]) {
  const bool up = bo >= 4u;
  const uint32_t a = up ? d[1] : d[0], b = up ? d[2] : d[1];
  const uint32_t sel = bo & 3u;
  const uint32_t lo = __builtin_amdgcn_alignbyte(b, a, sel);  // bytes bo..bo+3
  const uint32_t hi = b >> (8 * sel);                         // byte bo+4 in bits 0..7
  out[0] = (float)(lo & 0xffu);
  out[1] = (float)((lo >> 8) & 0xffu);
  out[2] = (float)((lo >> 16) & 0xffu);
  out[3] = (float)(lo >> 24);
  out[4] = (float)(hi & 0xffu);
}

// ---- window cache (template parameter WC) --------------------------------------------------------------
// The 5x5 window of the current image moves by a fraction of a pixel per Gauss-Newton iteration,
// yet re-fetching it every iteration misses L2 (128 resident problems per XCD x ~64 KB of touched
// sectors) and puts an HBM round trip on the critical path of every iteration.  With the cache a
// lane fetches 7 rows x 3 aligned dwords around the patch (49+ bytes, once) and later iterations
// cut their 5x5 window out of those 21 registers as long as the integer position stays within
// +-1 row and the 12 cached columns; only then is nothing loaded at all.
// v_cndmask_b32 with the lane mask in an SGPR pair.  The VOP2 form the compiler prefers reads VCC and
// issues ~3.6x slower on gfx950 (scripts/valu_ubench.hip: 10.7 against 2.95 SIMD cycles per
// wave-instruction); K1 spends 45 selects per patch and iteration on its window cache.
__device__ __forceinline__ uint32_t sel_e64(uint64_t mask, uint32_t if_set, uint32_t if_clear) {
#ifdef SIA_VCC_SELECT
  return ((mask >> (threadIdx.x & 63)) & 1) ? if_set : if_clear;
#else
  uint32_t r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(if_clear), "v"(if_set), "s"(mask));
  return r;
#endif
}
// bytes [bo, bo+4] (bo in 0..7) of three consecutive dwords as floats; up = lanes with bo >= 4
__device__ __forceinline__ void cut_row5(uint32_t a, uint32_t b, uint32_t c, int bo, uint64_t up, float out[5]) {
  const uint32_t d0 = sel_e64(up, b, a), d1 = sel_e64(up, c, b);
  const uint32_t sel = (uint32_t)(bo & 3);
  const uint32_t lo = __builtin_amdgcn_alignbyte(d1, d0, sel);
  const uint32_t hi = d1 >> (8 * sel);
  out[0] = (float)(lo & 0xffu);
  out[1] = (float)((lo >> 8) & 0xffu);
  out[2] = (float)((lo >> 16) & 0xffu);
  out[3] = (float)(lo >> 24);
  out[4] = (float)(hi & 0xffu);
}

__device__ __forceinline__ int sym6_rt(int i, int j) {
  const int a = i < j ? i : j, b = i < j ? j : i;
  return a * 6 - (a * (a - 1)) / 2 + (b - a);
}

// ---- the per-level arithmetic of a patch ---------------------------------------------------------------------------------
// H of one patch, J J' summed over its 16 pixels with J = dx a + dy b:
//     H_p = Sxx aa' + Sxy (ab' + ba') + Syy bb' = [a b] S [a b]'
// in the factored form: c = Sxx a + Sxy b, d = Sxy a + Syy b, H_p(i,j) = a_i c_j + b_i d_j -- about 50 multiply-adds where
// the three products per entry written out cost ~150, the same four terms per entry (it differs from the written-out form
// by rounding only).  a = fl * jac.row(0), b = fl * jac.row(1) of Frame::jacobian_xyz2uv: a[1] and b[0] are zero by construction
// and are NOT READ.  hp: the packed upper triangle in sym6 order.  A patch that is not part of the sum passes S = 0 and
// contributes exact zeros.
template <typename T>
__host__ __device__ __forceinline__ void sia_patch_hessian(const T a[6], const T b[6], T sxx, T sxy, T syy, T hp[21]) {
  // column by column: c_j and d_j are used up at once (only a, b and the finished entries stay live)
  hp[sym6(0, 0)] = a[0] * (sxx * a[0]);
  hp[sym6(0, 1)] = a[0] * (sxy * b[1]);
  hp[sym6(1, 1)] = b[1] * (syy * b[1]);
#pragma unroll
  for (int j = 2; j < 6; ++j) {
    const T cj = sxx * a[j] + sxy * b[j];
    const T dj = sxy * a[j] + syy * b[j];
    hp[sym6(0, j)] = a[0] * cj;
    hp[sym6(1, j)] = b[1] * dj;
#pragma unroll
    for (int i = 2; i <= j; ++i) hp[sym6(i, j)] = a[i] * cj + b[i] * dj;
  }
}

// The bilinear sample, with the order of its one multiplication and three fused multiply-adds spelled out: the template
// (sia_ref_tile_packed, the scalar block of sia_kernel) and the warped patch (every evaluation) must round alike -- a frame aligned
// against itself has residuals that are exactly zero -- and left to itself the compiler may fuse a*b + c*d either way
// round, differently for scalars and for register pairs.
__device__ __forceinline__ float sia_bilerp(float wtl, float wtr, float wbl, float wbr, float tl, float tr, float bl, float br) {
  return __builtin_fmaf(wbr, br, __builtin_fmaf(wbl, bl, __builtin_fmaf(wtr, tr, wtl * tl)));
}
typedef float sia_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ sia_f2 sia_bilerp2(sia_f2 wtl, sia_f2 wtr, sia_f2 wbl, sia_f2 wbr, sia_f2 tl, sia_f2 tr, sia_f2 bl,
                                              sia_f2 br) {
  return __builtin_elementwise_fma(wbr, br, __builtin_elementwise_fma(wbl, bl, __builtin_elementwise_fma(wtr, tr, wtl * tl)));
}

// The bilinear weights.  The reference forms these products in double and rounds to float (:118-121, :200-203).  u >= 3
// here, so su and sv are multiples of 2^-22: 1-su and 1-sv are exact in f32, and the f32 product of two f32 values is
// the correctly rounded exact product, like the rounded double product -- bit-identical.
__device__ __forceinline__ void sia_weights(float su, float sv, float& wtl, float& wtr, float& wbl, float& wbr) {
  wtl = (1.f - su) * (1.f - sv);
  wtr = su * (1.f - sv);
  wbl = (1.f - su) * sv;
  wbr = su * sv;
}

// bytes [bo, bo+6] of a 12-byte run as the column pairs (0,2) (1,3) (2,4) (3,5) (4,5) (5,6) the packed samples read
__device__ __forceinline__ void sia_cut_row7_pairs(const uint32_t d[3], uint32_t bo, sia_f2 p[6]) {
  float w[7];
  cut_row7(d, bo, w);
  p[0] = sia_f2{w[0], w[2]};
  p[1] = sia_f2{w[1], w[3]};
  p[2] = sia_f2{w[2], w[4]};
  p[3] = sia_f2{w[3], w[5]};
  p[4] = sia_f2{w[4], w[5]};
  p[5] = sia_f2{w[5], w[6]};
}
__device__ __forceinline__ float4 sia_f4(sia_f2 a, sia_f2 b) { return make_float4(a.x, a.y, b.x, b.y); }

// precomputeReferencePatches of one patch (sparse_img_align.cpp:84-145) for the packed pixel loop, from its 7 x 7 window
// (seven 12-byte runs rw, the window's first byte at offset rbo in them, the sub-pixel position su, sv): the 6 x 6
// neighbourhood of bilinear samples without its corners, handed to store(k, float4) as the eight float4 of the workgroup
// kernel's LDS tile -- rows 1-4 as the column pairs (0,2) (1,3) (4,5), rows 0 and 5 as (1,3) (2,4) -- and the sums Sxx, Sxy,
// Syy of the products of the central-difference gradients dx, dy over the 4 x 4 patch.
// Two columns per instruction: sia_bilerp2 does per sample the operations of sia_bilerp in the same order (the same bits).
// The gradients are formed two per instruction too and WITHOUT their factor 0.5: it only feeds the three sums, a power of two
// commutes with every rounding of a 16-term sum (|difference| <= 255: nothing overflows or goes subnormal), so the sums of
// the unscaled products times 0.25 are the same bits.  The sums keep their order: y outer, x inner, one accumulator each.
// Rows slide (tile rows r-2, r-1, r are live while row r is sampled; a float4 is stored as soon as its rows exist).
// acc + a * b of the three sums as the scalar block's `S += dx * dy` is compiled: on the device contracted into one fused
// multiply-add (every one of its 48 is a v_fmac_f32), on the host (-ffp-contract=off) a product and a sum.  Spelled out,
// because the compiler does not contract a product it has first put back together from the halves of two register pairs.
// The first two squares of Sxx and of Syy are the exception: `0 + a0 * a0` folds to the product (a square has no negative
// zero to lose), and of the two products of a0 * a0 + a1 * a1 the device compiler rounds the SECOND and fuses the first --
// fma(a0, a0, a1 * a1), where the chain would be fma(a1, a1, a0 * a0).  Sxy's first sum keeps its zero and chains normally.
#ifdef SVO_HOST_MATH_TEST
#define SIA_SUM_PRODUCT(a, b, acc) ((acc) + (a) * (b))
#define SIA_SUM_SQUARES_START(a0, a1) ((a0) * (a0) + (a1) * (a1))
#else
#define SIA_SUM_PRODUCT(a, b, acc) __builtin_fmaf((a), (b), (acc))
#define SIA_SUM_SQUARES_START(a0, a1) __builtin_fmaf((a0), (a0), (a1) * (a1))
#endif
template <typename STORE>
__device__ __forceinline__ void sia_ref_tile_packed(const uint32_t rw[7][3], uint32_t rbo, float su, float sv, STORE&& store,
                                                    float& Sxx, float& Sxy, float& Syy) {
  float wtl, wtr, wbl, wbr;
  sia_weights(su, sv, wtl, wtr, wbl, wbr);
  const sia_f2 vtl = sia_f2{wtl, wtl}, vtr = sia_f2{wtr, wtr}, vbl = sia_f2{wbl, wbl}, vbr = sia_f2{wbr, wbr};
  const sia_f2 z2 = sia_f2{0.f, 0.f};
  float sxx = 0.f, sxy = 0.f, syy = 0.f;
  sia_f2 wp[6], wn[6];                             // window rows r, r + 1
  sia_f2 p13 = z2, p24 = z2;                       // tile row r - 2: columns (1,3) (2,4)
  sia_f2 m02 = z2, m13 = z2, m24 = z2, m45 = z2;   // tile row r - 1
  sia_cut_row7_pairs(rw[0], rbo, wp);
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    sia_cut_row7_pairs(rw[r + 1], rbo, wn);
    sia_f2 n02 = z2, n13, n24, n45 = z2;  // tile row r
    if (r == 0 || r == 5) {
      n13 = sia_bilerp2(vtl, vtr, vbl, vbr, wp[1], wp[2], wn[1], wn[2]);
      n24 = sia_bilerp2(vtl, vtr, vbl, vbr, wp[2], wp[3], wn[2], wn[3]);
    } else {
      n02 = sia_bilerp2(vtl, vtr, vbl, vbr, wp[0], wp[1], wn[0], wn[1]);
      n13 = sia_bilerp2(vtl, vtr, vbl, vbr, wp[1], wp[2], wn[1], wn[2]);
      n45 = sia_bilerp2(vtl, vtr, vbl, vbr, wp[4], wp[5], wn[4], wn[5]);
      n24 = sia_f2{n02.y, n45.x};
    }
    if (r == 0) store(0, sia_f4(n13, n24));
    if (r == 1) store(1, sia_f4(n02, n13));
    if (r == 2) { store(2, sia_f4(m45, n02)); store(3, sia_f4(n13, n45)); }
    if (r == 3) store(4, sia_f4(n02, n13));
    if (r == 4) { store(5, sia_f4(m45, n02)); store(6, sia_f4(n13, n45)); }
    if (r == 5) store(7, sia_f4(n13, n24));
    if (r >= 2) {
      // patch row y = r - 2: dx from tile row r - 1, dy = tile row r minus tile row r - 2 (twice the central differences)
      const sia_f2 m35 = sia_f2{m13.y, m45.y};
      const sia_f2 dxa = m24 - m02, dxb = m35 - m13;  // pixels x = 0, 2 and x = 1, 3
      const sia_f2 dya = n13 - p13, dyb = n24 - p24;
      const float dx[4] = {dxa.x, dxb.x, dxa.y, dxb.y}, dy[4] = {dya.x, dyb.x, dya.y, dyb.y};
      if (r == 2) {  // (the sums are zero)
        sxx = SIA_SUM_SQUARES_START(dx[0], dx[1]);
        syy = SIA_SUM_SQUARES_START(dy[0], dy[1]);
        sxy = SIA_SUM_PRODUCT(dx[1], dy[1], SIA_SUM_PRODUCT(dx[0], dy[0], sxy));
      }
#pragma unroll
      for (int x = (r == 2 ? 2 : 0); x < 4; ++x) {
        sxx = SIA_SUM_PRODUCT(dx[x], dx[x], sxx);
        sxy = SIA_SUM_PRODUCT(dx[x], dy[x], sxy);
        syy = SIA_SUM_PRODUCT(dy[x], dy[x], syy);
      }
    }
    p13 = m13; p24 = m24;
    m02 = n02; m13 = n13; m24 = n24; m45 = n45;
#pragma unroll
    for (int k = 0; k < 6; ++k) wp[k] = wn[k];
    asm volatile("" ::: "memory");  // keeps the compiler from cutting all seven window rows up front
  }
  Sxx = 0.25f * sxx;
  Sxy = 0.25f * sxy;
  Syy = 0.25f * syy;
}

// ---- what both kernels do the same way, once ---------------------------------------------------------------------------
// sparse_img_align.cpp:47-51: nothing to track, pose untouched (one lane of the frame writes)
__device__ __forceinline__ void sia_untracked(const SiaArgs& a, int b) {
  for (int k = 0; k < 12; ++k) a.T_out[12 * b + k] = a.T_in[12 * b + k];
  if (a.H_out)
    for (int k = 0; k < 36; ++k) a.H_out[36 * b + k] = 0.0;
  a.n_tracked[b] = 0;
  if (a.iters)
    for (int k = 0; k < SVO_HIP_MAX_LEVELS; ++k) a.iters[SVO_HIP_MAX_LEVELS * b + k] = 0;
  if (a.chi2) a.chi2[b] = 1e10;
  if (a.status) a.status[b] = 0;
}

// pyramid geometry per level in LDS (copied from the kernel arguments so that the level loop can index it dynamically;
// the six-line copy loop stays in each kernel: as a function it cost sia_kernel<256, true, false, 1> a VGPR, profiles/r10a_*)
struct SiaLevels {
  long long lo[SVO_HIP_MAX_LEVELS];
  int lw[SVO_HIP_MAX_LEVELS], lh[SVO_HIP_MAX_LEVELS], lp[SVO_HIP_MAX_LEVELS];
};

// The model a frame starts from: T_in (rotation row-major, then translation) as the unit quaternion Sophus stores, and the
// rotation matrix of that quaternion (what every later update produces).  Every lane computes the same values.
__device__ __forceinline__ void sia_model_init(const double* T, double q[4], double R[9], double tr[3]) {
  for (int k = 0; k < 9; ++k) R[k] = T[k];
  for (int k = 0; k < 3; ++k) tr[k] = T[9 + k];
  quat_from_R(R, q);
  quat_to_R(q, R);
}

// the camera of a distorted model from the kernel's parameter block
__device__ __forceinline__ Cam sia_cam(const svo_hip_sia_params& P) {
  Cam cm;
  cm.fx = P.fx; cm.fy = P.fy; cm.cx = P.cx; cm.cy = P.cy;
  cm.width = 0; cm.height = 0;
  cm.model = P.cam_model;
#pragma unroll
  for (int k = 0; k < 5; ++k) cm.d[k] = P.d[k];
  return cm;
}
// cam_->world2cam(project2d(T * xyz)) (:183) at level 0, one reciprocal (fast_rcp: the IEEE division sequence sits on
// the critical path of every iteration).  DIST: a distorted model (radial-tangential pinhole or ATAN); the undistorted
// pinhole keeps its own instantiation so that its inner loop carries no model dispatch.
template <bool DIST>
__device__ __forceinline__ void sia_project(const svo_hip_sia_params& P, const double R[9], const double tr[3], double X, double Y,
                                            double Z, double& pu, double& pv) {
  const double xc = R[0] * X + R[1] * Y + R[2] * Z + tr[0];
  const double yc = R[3] * X + R[4] * Y + R[5] * Z + tr[1];
  const double zc = R[6] * X + R[7] * Y + R[8] * Z + tr[2];
  const double izc = fast_rcp(zc);
  if (DIST) {
    const Cam cm = sia_cam(P);
    const double uvn[2] = {xc * izc, yc * izc};
    double pxd[2];
    world2cam_uv(cm, uvn, pxd);
    pu = pxd[0];
    pv = pxd[1];
  } else {
    pu = P.fx * (xc * izc) + P.cx;
    pv = P.fy * (yc * izc) + P.cy;
  }
}
// the 4 x 4 patch and its bilinear neighbours 3 px inside the level (fu, fv: floored position; NaN / huge coordinates fail
// the comparisons like the reference's int tests do)
__device__ __forceinline__ bool sia_inside3(float fu, float fv, int cols, int rows) {
  return fu - 3.f >= 0.f && fv - 3.f >= 0.f && fu + 3.f < (float)cols && fv + 3.f < (float)rows;
}

// The window cache of one patch (see above): rows = 7 runs of 12 bytes of the current level, columns [u0, u0+11], rows
// [v0, v0+6]; v0 = -100000 while it is empty.  (Free functions over the caller's own registers: as members of a struct
// they moved sia_kernel's register allocation, profiles/r10a_*.)  ROWS = 1: an instantiation without the cache.
// sia_wave_kernel calls the two below; sia_kernel keeps the same lines written out in its iteration (with the calls it
// measured slower, r10a section 4).
// r0 (0..2), bo (0..7): the first cached row / byte of the 5 x 5 window around (u_i, v_i); fetched again when the window
// has moved out of the cache
template <int ROWS>
__device__ __forceinline__ void sia_wc_seek(uint32_t (&rows)[ROWS][3], int& u0, int& v0, const uint8_t* cur_img, int pitch,
                                            int u_i, int v_i, int& r0, int& bo) {
  r0 = (v_i - 2) - v0;
  bo = (u_i - 2) - u0;
  if (!(r0 >= 0 && r0 <= 2 && bo >= 0 && bo <= 7)) {
    v0 = v_i - 3;
    u0 = run_start(u_i - 3, 7);
    load_window12<ROWS>(cur_img, pitch, u0, v0, rows);
    r0 = 1;
    bo = (u_i - 2) - u0;
  }
}
// window row r (0..4) as five floats; k0 / k1 / kup: the lanes with r0 == 0 / r0 == 1 / bo >= 4
template <int ROWS>
__device__ __forceinline__ void sia_wc_row(const uint32_t (&rows)[ROWS][3], int r, uint64_t k0, uint64_t k1, uint64_t kup, int bo,
                                           float out[5]) {
  constexpr int S = ROWS == 7 ? 1 : 0;  // keeps the indices in range when the cache is compiled out
  const uint32_t d0 = sel_e64(k0, rows[r * S][0], sel_e64(k1, rows[(r + 1) * S][0], rows[(r + 2) * S][0]));
  const uint32_t d1 = sel_e64(k0, rows[r * S][1], sel_e64(k1, rows[(r + 1) * S][1], rows[(r + 2) * S][1]));
  const uint32_t d2 = sel_e64(k0, rows[r * S][2], sel_e64(k1, rows[(r + 1) * S][2], rows[(r + 2) * S][2]));
  cut_row5(d0, d1, d2, bo, kup, out);
}

// The 6 x 6 tile of interpolated reference samples without its corners <-> the eight float4 of its LDS slot (slot(k): a
// reference to the k-th float4), in plain order
//   q0 = r0 c1..4 | q1 = r1 c0..3 | q2 = r1 c4,5 r2 c0,1 | q3 = r2 c2..5
//   q4 = r3 c0..3 | q5 = r3 c4,5 r4 c0,1 | q6 = r4 c2..5 | q7 = r5 c1..4
// and in the order the packed pixel loop pairs the columns (sia_ref_tile_packed).
template <typename SLOT>
__device__ __forceinline__ void sia_tile_store(const float Bt[6][6], SLOT&& slot) {
  slot(0) = make_float4(Bt[0][1], Bt[0][2], Bt[0][3], Bt[0][4]);
  slot(1) = make_float4(Bt[1][0], Bt[1][1], Bt[1][2], Bt[1][3]);
  slot(2) = make_float4(Bt[1][4], Bt[1][5], Bt[2][0], Bt[2][1]);
  slot(3) = make_float4(Bt[2][2], Bt[2][3], Bt[2][4], Bt[2][5]);
  slot(4) = make_float4(Bt[3][0], Bt[3][1], Bt[3][2], Bt[3][3]);
  slot(5) = make_float4(Bt[3][4], Bt[3][5], Bt[4][0], Bt[4][1]);
  slot(6) = make_float4(Bt[4][2], Bt[4][3], Bt[4][4], Bt[4][5]);
  slot(7) = make_float4(Bt[5][1], Bt[5][2], Bt[5][3], Bt[5][4]);
}
template <typename SLOT>
__device__ __forceinline__ void sia_tile_store_packed(const float Bt[6][6], SLOT&& slot) {
  slot(0) = make_float4(Bt[0][1], Bt[0][3], Bt[0][2], Bt[0][4]);
  slot(1) = make_float4(Bt[1][0], Bt[1][2], Bt[1][1], Bt[1][3]);
  slot(2) = make_float4(Bt[1][4], Bt[1][5], Bt[2][0], Bt[2][2]);
  slot(3) = make_float4(Bt[2][1], Bt[2][3], Bt[2][4], Bt[2][5]);
  slot(4) = make_float4(Bt[3][0], Bt[3][2], Bt[3][1], Bt[3][3]);
  slot(5) = make_float4(Bt[3][4], Bt[3][5], Bt[4][0], Bt[4][2]);
  slot(6) = make_float4(Bt[4][1], Bt[4][3], Bt[4][4], Bt[4][5]);
  slot(7) = make_float4(Bt[5][1], Bt[5][3], Bt[5][2], Bt[5][4]);
}
// (plain order; the four corners come back as zero)
template <typename SLOT>
__device__ __forceinline__ void sia_tile_load(SLOT&& slot, float Bt[6][6]) {
  const float4 q0 = slot(0), q1 = slot(1), q2 = slot(2), q3 = slot(3);
  const float4 q4 = slot(4), q5 = slot(5), q6 = slot(6), q7 = slot(7);
  Bt[0][0] = Bt[0][5] = Bt[5][0] = Bt[5][5] = 0.f;
  Bt[0][1] = q0.x; Bt[0][2] = q0.y; Bt[0][3] = q0.z; Bt[0][4] = q0.w;
  Bt[1][0] = q1.x; Bt[1][1] = q1.y; Bt[1][2] = q1.z; Bt[1][3] = q1.w;
  Bt[1][4] = q2.x; Bt[1][5] = q2.y; Bt[2][0] = q2.z; Bt[2][1] = q2.w;
  Bt[2][2] = q3.x; Bt[2][3] = q3.y; Bt[2][4] = q3.z; Bt[2][5] = q3.w;
  Bt[3][0] = q4.x; Bt[3][1] = q4.y; Bt[3][2] = q4.z; Bt[3][3] = q4.w;
  Bt[3][4] = q5.x; Bt[3][5] = q5.y; Bt[4][0] = q5.z; Bt[4][1] = q5.w;
  Bt[4][2] = q6.x; Bt[4][3] = q6.y; Bt[4][4] = q6.z; Bt[4][5] = q6.w;
  Bt[5][1] = q7.x; Bt[5][2] = q7.y; Bt[5][3] = q7.z; Bt[5][4] = q7.w;
}

// a = fl * jac.row(0), b = fl * jac.row(1) of Frame::jacobian_xyz2uv (frame.h:116-138) from the normalised coordinates
// (x/z, y/z, 1/z) of xyz_ref.  The callers hand over opaque copies of zi / xn / yn (an empty asm): otherwise these
// products, all invariant in the iteration loop, are hoisted out of it and stay live across it.
template <typename T>
__device__ __forceinline__ void sia_jac_rows(T zi, T xn, T yn, T fl, T ja[6], T jb[6]) {
  const T one = 1, zero = 0;
  ja[0] = -zi * fl; ja[1] = zero; ja[2] = xn * zi * fl; ja[3] = xn * yn * fl; ja[4] = -(one + xn * xn) * fl; ja[5] = yn * fl;
  jb[0] = zero; jb[1] = -zi * fl; jb[2] = yn * zi * fl; jb[3] = (one + yn * yn) * fl; jb[4] = -xn * yn * fl; jb[5] = -xn * fl;
}
// What a patch adds to an evaluation's eight sums: Jres -= J res with J = dx a + dy b (gx / gy: the patch's sums of res dx and
// res dy without the central difference's factor 0.5), chi2 (c2), n_meas.  m: the patch lies inside the current image;
// gmask: 0 while its Jacobian columns are zero at this level.  (sia_kernel keeps these lines written out, as the window
// cache above; tests/host/k1_level_arith_main.cpp holds this function to that formula bit for bit.)
template <typename T>
__device__ __forceinline__ void sia_jres_partials(T zi, T xn, T yn, T fl, T gmask, bool m, T gx, T gy, float c2, T part[8]) {
  const T gsc = (T)0.5 * fl * gmask;
  const T gxf = m ? gx * gsc : (T)0, gyf = m ? gy * gsc : (T)0;
  part[0] = zi * gxf;
  part[1] = zi * gyf;
  part[2] = -zi * (xn * gxf + yn * gyf);
  part[3] = -(xn * yn * gxf + ((T)1 + yn * yn) * gyf);
  part[4] = ((T)1 + xn * xn) * gxf + xn * yn * gyf;
  part[5] = xn * gyf - yn * gxf;
  part[6] = (T)c2;
  part[7] = m ? (T)16 : (T)0;
}

// H^-1 of the packed upper triangle H by Gauss-Jordan on a 6 x 6 tile held one element per lane (36 lanes of one wave;
// every lane of the wave calls), LDS (A: scratch, Hinv: the result, row-major) as the row / column exchange: a few
// registers instead of the ~90 a register LDL^T keeps live.  Same-wave LDS traffic: DS instructions of one wave execute
// in order; the wavefront-scope fences stop the compiler from moving accesses across the exchanges.  A zero pivot
// contributes nothing, like the D^-1 step of Eigen's LDLT::solve.
// (fast_rcp, not 1.0 / p: six dependent divisions per rebuild of H^-1 -- K1 1.220 -> 1.207 ms together with the patch's
// normalised coordinates, profiles/r06ah_*)
__device__ __forceinline__ void sia_gauss_jordan6(const double* H, double* A, double* Hinv, int lane) {
  const int gi = lane / 6, gj = lane - 6 * gi;
  if (lane < 36) {
    A[lane] = H[sym6_rt(gi, gj)];
    Hinv[lane] = (gi == gj) ? 1.0 : 0.0;
  }
  for (int k = 0; k < 6; ++k) {
    SVO_WAVE_LDS_FENCE();
    if (lane < 36) {
      const double p = A[k * 6 + k];
      const double aik = A[gi * 6 + k];
      const double akj = A[k * 6 + gj];
      const double bkj = Hinv[k * 6 + gj];
      const double aij = A[lane];
      const double bij = Hinv[lane];
      const double ip = (fabs(p) > 2.2250738585072014e-308) ? fast_rcp(p) : 0.0;
      const double na = (gi == k) ? akj * ip : aij - aik * (akj * ip);
      const double nb = (gi == k) ? bkj * ip : bij - aik * (bkj * ip);
      SVO_LANES_LDS_FENCE();
      A[lane] = na;
      Hinv[lane] = nb;
    }
  }
}
// x_ = H_.ldlt().solve(Jres_) (:247), here x = H^-1 Jres from the wave-uniform totals b0..b5: lane i (< 6) holds x_i
__device__ __forceinline__ double sia_solve_rows(const double* Hinv, double b0, double b1, double b2, double b3, double b4, double b5,
                                                 int lane) {
  const double* row = &Hinv[6 * (lane < 6 ? lane : 0)];
  return row[0] * b0 + row[1] * b1 + row[2] * b2 + row[3] * b3 + row[4] * b4 + row[5] * b5;
}
// vk::norm_max(x_)
__device__ __forceinline__ double sia_norm_max6(double x0, double x1, double x2, double x3, double x4, double x5) {
  return fmax(fmax(fmax(fabs(x0), fabs(x1)), fmax(fabs(x2), fabs(x3))), fmax(fabs(x4), fabs(x5)));
}

// sparse_align_wave.hip
int launch_sia_wave(const SiaArgs& args, int B, hipStream_t s);
bool sia_wave_applies(const SiaArgs& args, int B);

}  // namespace svo_sia
