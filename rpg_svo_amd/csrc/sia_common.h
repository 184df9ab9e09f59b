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

// 1 / z as v_rcp_f64 + two Newton steps (the IEEE division sequence is three times as long; K1 is a tolerance-mode kernel
// and its agreement with the reference's translation unit is the same to six digits either way: profiles/r06ah_*)
__device__ __forceinline__ double sia_rcp(double z) {
  double r = __builtin_amdgcn_rcp(z);
  r = fma(fma(-z, r, 1.0), r, r);
  r = fma(fma(-z, r, 1.0), r, r);
  return r;
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

// a wave-uniform value read back through v_readfirstlane: its dwords stay in SGPRs instead of VGPRs
__device__ __forceinline__ double sia_uni(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
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
  // The reference forms these products in double and rounds to float (:118-121).  u >= 3 here, so su
  // and sv are multiples of 2^-22: 1-su and 1-sv are exact in f32, and the f32 product of two f32
  // values is the correctly rounded exact product, like the rounded double product -- bit-identical.
  const float wtl = (1.f - su) * (1.f - sv);
  const float wtr = su * (1.f - sv);
  const float wbl = (1.f - su) * sv;
  const float wbr = su * sv;
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

// sparse_align_wave.hip
int launch_sia_wave(const SiaArgs& args, int B, hipStream_t s);
bool sia_wave_applies(const SiaArgs& args, int B);

}  // namespace svo_sia
