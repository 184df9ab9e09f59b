// klt_track.hip -- K8: the tracking half of the two-view bootstrap on the device.
//
// Replaces initialization::trackKlt (svo/src/initialization.cpp:127-169: cv::calcOpticalFlowPyrLK with a 30 x 30 window,
// 4 pyramid levels above level 0, 30 iterations / eps 0.001, OPTFLOW_USE_INITIAL_FLOW, then bearings and disparities of
// the surviving points) and the gating numbers of KltHomographyInit::addSecondFrame (:48-53: number tracked, vk::getMedian
// of the disparities).  The tracker is Bouguet's pyramidal Lucas-Kanade as OpenCV's documentation states it, in f32,
// on the tiled pyramid store this library builds (vk::halfSample levels, no padding: every pixel fetch clamps its
// coordinates to the level, i.e. the level is continued by its border pixels, and the Scharr derivatives are those of
// the continued image).  include/svo_hip.h states the specification; tests/klt_checker.py restates it in f64.
//
//   klt_track_kernel      one wave64 per (pair, point), carried through all levels.  The 30 x 30 window is 900 pixels
//                         = 15 per lane on 60 lanes: lane l owns window row l / 2, columns 15 (l & 1) .. + 14.  Its
//                         bilinear samples need 16 bytes of two adjacent image rows (four rows x 18 bytes for the
//                         derivatives of the template), fetched as aligned dwords -- which never cross a tile row of
//                         the store (pyr_addr.h) -- and shifted into place with v_alignbyte; a run that touches the
//                         border is fetched byte by byte with clamped coordinates.  I, Ix, Iy of the template stay in
//                         45 VGPRs per lane for the level's iterations: no LDS.  The sums (a11, a12, a22 once per
//                         level; b1, b2 per iteration; the residual once) are 15 terms per lane in window order and
//                         then wave_reduce.h's exchange tree: a fixed order, the same bits on every run.  Every
//                         decision is taken on wave-uniform values, so the wave never diverges on control flow.
//   klt_summarize_kernel  one workgroup per pair: bearing and disparity per tracked point, their number, and the median
//                         disparity by block_select.h's rank counting (the element of rank n / 2 is a value, whatever
//                         algorithm finds it).
#pragma clang fp contract(off)
#include "block_select.h"
#include "capi_common.h"
#include "track_math.h"
#include "wave_reduce.h"

using namespace svo_capi;
using namespace svo_dev;

namespace {

// The tracker's arithmetic may contract a * b + c into one fused multiply-add (the bilinear samples and the window sums
// are chains of them: 4 instructions per sample instead of 7): its specification is an f64 restatement with a tolerance,
// not the bits of another f32 implementation.  The summary kernel further down goes back to separate roundings, because
// its bearings are svo_hip_cam2world's bits (track_math.h).
#pragma clang fp contract(fast)

constexpr int KLT_WIN = 30;                 // the window the kernel implements
constexpr int KLT_PER_LANE = 15;            // pixels of one window row a lane owns
constexpr int KLT_LANES = 60;               // lanes that own pixels
constexpr float KLT_HALF = 14.5f;           // (KLT_WIN - 1) / 2
constexpr float KLT_FLT_EPSILON = 1.1920929e-07f;

struct KltArgs {
  svo_hip_pyr_layout L;
  const uint8_t* store;
  const int32_t* ref_slot;  // [n_pairs]
  const int32_t* cur_slot;  // [n_pairs]
  int n_pts;
  const float* px_ref;      // [n_pairs][n_pts][2]
  float* px_cur;            // [n_pairs][n_pts][2] in: initial flow, out
  uint8_t* status;          // [n_pairs][n_pts] in/out
  float* error;             // [n_pairs][n_pts]
  int max_level, max_iter;
  float eps2, min_eig_threshold;
};

// N consecutive pixels xs .. xs + N - 1 of row y of a level as floats, coordinates clamped to the level.
// Inside the level: ceil(N / 4) + 1 aligned dwords (an aligned dword never crosses a tile row), realigned by xs & 3.
template <int N>
__device__ __forceinline__ void load_row(const uint8_t* __restrict__ lvl, int w, int h, int pitch, int xs, int y, float out[N]) {
  constexpr int NA = (N + 3) / 4, ND = NA + 1;
  const uint32_t ro = svo_pyr::row_off(min(max(y, 0), h - 1), pitch);
  const int xa = xs & ~3;
  if (xs >= 0 && xs + N <= w && xa + 4 * ND <= pitch) {
    uint32_t d[ND];
#pragma unroll
    for (int m = 0; m < ND; ++m) d[m] = svo_pyr::ld32(lvl, ro + svo_pyr::col_off(xa + 4 * m));
    const uint32_t sb = (uint32_t)(xs & 3);
#pragma unroll
    for (int m = 0; m < NA; ++m) {
      const uint32_t v = __builtin_amdgcn_alignbyte(d[m + 1], d[m], sb);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * m + k < N) out[4 * m + k] = (float)((v >> (8 * k)) & 0xffu);
    }
  } else {
#pragma unroll
    for (int k = 0; k < N; ++k) out[k] = (float)lvl[ro + svo_pyr::col_off(min(max(xs + k, 0), w - 1))];
  }
}

// wave totals of v[0 .. NV-1] (NV <= 8) on every lane, as wave-uniform values
template <int NV>
__device__ __forceinline__ void wave_sums(const float part[NV], int lane, float out[NV]) {
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = k < NV ? part[k] : 0.0f;
  const float t = wave_reduce8(v, lane);  // lanes 8g .. 8g+7 hold the total of v[g]
#pragma unroll
  for (int k = 0; k < NV; ++k) out[k] = readlane_f32(t, 8 * k);
}

// floor(t) as an int when -KLT_WIN <= floor(t) < size (the window's corner is close enough to the level), else false
__device__ __forceinline__ bool corner_ok(float t, int size, int& i) {
  const float f = floorf(t);
  if (!(f >= (float)-KLT_WIN && f < (float)size)) return false;  // (also NaN / infinity)
  i = (int)f;
  return true;
}

struct Bilinear {
  float w00, w01, w10, w11;
  __device__ __forceinline__ Bilinear(float ax, float ay)
      : w00((1.0f - ax) * (1.0f - ay)), w01(ax * (1.0f - ay)), w10((1.0f - ax) * ay), w11(ax * ay) {}
  __device__ __forceinline__ float operator()(float v00, float v01, float v10, float v11) const {
    return w00 * v00 + w01 * v01 + w10 * v10 + w11 * v11;
  }
};

// J - I of the lane's 15 pixels with the window's corner at (x0 + ax, y0 + ay) of level `lvl`
__device__ __forceinline__ void sample_diff(const uint8_t* __restrict__ lvl, int w, int h, int pitch, int x0, int y0,
                                            float ax, float ay, const float I[KLT_PER_LANE], float diff[KLT_PER_LANE]) {
  float r0[KLT_PER_LANE + 1], r1[KLT_PER_LANE + 1];
  load_row<KLT_PER_LANE + 1>(lvl, w, h, pitch, x0, y0, r0);
  load_row<KLT_PER_LANE + 1>(lvl, w, h, pitch, x0, y0 + 1, r1);
  const Bilinear bil(ax, ay);
#pragma unroll
  for (int j = 0; j < KLT_PER_LANE; ++j) diff[j] = bil(r0[j], r0[j + 1], r1[j], r1[j + 1]) - I[j];
}

// Four waves per SIMD (128 VGPRs, no scratch): a wave's evaluations are a chain of gather -> sums -> exchange -> step, and
// the fourth wave covers more of it than the 136 registers the compiler would otherwise take buy (33.8 against 36.3 ms on
// 4096 pairs x 352 points).
__global__ void __launch_bounds__(64, 4) klt_track_kernel(const KltArgs a) {
  const unsigned item = xcd_contiguous_block();  // the points of a pair share two slots: neighbours on one XCD's L2
  const int lane = (int)threadIdx.x;
  if (a.status[item] == 0) return;  // lost points stay lost, nothing of theirs is written
  const int pair = (int)(item / (unsigned)a.n_pts);
  const uint8_t* ref = a.store + (int64_t)a.ref_slot[pair] * a.L.slot_bytes;
  const uint8_t* cur = a.store + (int64_t)a.cur_slot[pair] * a.L.slot_bytes;
  const float prx = a.px_ref[2 * (size_t)item], pry = a.px_ref[2 * (size_t)item + 1];
  const float top = 1.0f / (float)(1 << a.max_level);
  float qx = a.px_cur[2 * (size_t)item] * top, qy = a.px_cur[2 * (size_t)item + 1] * top;
  // lanes 60..63 own no pixel: they walk row 29 again and contribute zeros
  const bool owner = lane < KLT_LANES;
  const int wi = min(lane >> 1, KLT_WIN - 1), wj = (lane & 1) * KLT_PER_LANE;
  bool tracked = true;
  float err = 0.0f;

  for (int l = a.max_level; l >= 0 && tracked; --l) {
    if (l != a.max_level) { qx *= 2.0f; qy *= 2.0f; }
    const int w = a.L.w[l], h = a.L.h[l], pitch = a.L.pitch[l];
    const uint8_t* lr = ref + a.L.offset[l];
    const uint8_t* lc = cur + a.L.offset[l];
    const float s = 1.0f / (float)(1 << l);
    const float tx = prx * s - KLT_HALF, ty = pry * s - KLT_HALF;
    int px0, py0;
    if (!corner_ok(tx, w, px0) || !corner_ok(ty, h, py0)) {
      if (l == 0) tracked = false;
      continue;
    }
    // ---- template: I, Ix, Iy of the lane's 15 pixels, and the structure tensor ------------------------------------
    float I[KLT_PER_LANE], Ix[KLT_PER_LANE], Iy[KLT_PER_LANE];
    {
      constexpr int NC = KLT_PER_LANE + 3;  // columns x - 1 .. x + 16
      float r0[NC], r1[NC], r2[NC], r3[NC];
      const int xs = px0 + wj - 1, y = py0 + wi;
      load_row<NC>(lr, w, h, pitch, xs, y - 1, r0);
      load_row<NC>(lr, w, h, pitch, xs, y, r1);
      load_row<NC>(lr, w, h, pitch, xs, y + 1, r2);
      load_row<NC>(lr, w, h, pitch, xs, y + 2, r3);
      const Bilinear bil(tx - (float)px0, ty - (float)py0);
      // Scharr responses (x 32) at the 16 columns of image rows y and y + 1, one column at a time: a pixel's samples
      // need the responses of its own column and the next, so nothing but the previous column's four values is kept
      float pxa = 0.0f, pya = 0.0f, pxb = 0.0f, pyb = 0.0f;
#pragma unroll
      for (int k = 0; k <= KLT_PER_LANE; ++k) {
        const float d0 = r0[k + 2] - r0[k], d1 = r1[k + 2] - r1[k], d2 = r2[k + 2] - r2[k], d3 = r3[k + 2] - r3[k];
        const float sxa = 3.0f * d0 + 10.0f * d1 + 3.0f * d2;
        const float sxb = 3.0f * d1 + 10.0f * d2 + 3.0f * d3;
        const float sya = 3.0f * (r2[k] - r0[k]) + 10.0f * (r2[k + 1] - r0[k + 1]) + 3.0f * (r2[k + 2] - r0[k + 2]);
        const float syb = 3.0f * (r3[k] - r1[k]) + 10.0f * (r3[k + 1] - r1[k + 1]) + 3.0f * (r3[k + 2] - r1[k + 2]);
        if (k > 0) {
          const int j = k - 1;
          I[j] = bil(r1[j + 1], r1[j + 2], r2[j + 1], r2[j + 2]);
          Ix[j] = bil(pxa, sxa, pxb, sxb) * 0.03125f;
          Iy[j] = bil(pya, sya, pyb, syb) * 0.03125f;
        }
        pxa = sxa; pya = sya; pxb = sxb; pyb = syb;
      }
    }
    float part[3] = {0.0f, 0.0f, 0.0f}, A[3];
#pragma unroll
    for (int j = 0; j < KLT_PER_LANE; ++j) {
      part[0] += Ix[j] * Ix[j];
      part[1] += Ix[j] * Iy[j];
      part[2] += Iy[j] * Iy[j];
    }
    if (!owner) part[0] = part[1] = part[2] = 0.0f;
    wave_sums<3>(part, lane, A);
    const float a11 = A[0], a12 = A[1], a22 = A[2];
    const float D = a11 * a22 - a12 * a12;
    const float min_eig = (a11 + a22 - sqrtf((a11 - a22) * (a11 - a22) + 4.0f * a12 * a12)) / (float)(2 * KLT_WIN * KLT_WIN);
    if (min_eig < a.min_eig_threshold || D < KLT_FLT_EPSILON) {
      if (l == 0) tracked = false;
      continue;
    }
    // ---- iterations ------------------------------------------------------------------------------------------------
    float pdx = 0.0f, pdy = 0.0f;
    for (int it = 0; it < a.max_iter; ++it) {
      const float ux = qx - KLT_HALF, uy = qy - KLT_HALF;
      int x0, y0;
      if (!corner_ok(ux, w, x0) || !corner_ok(uy, h, y0)) {
        if (l == 0) tracked = false;
        break;
      }
      float diff[KLT_PER_LANE];
      sample_diff(lc, w, h, pitch, x0 + wj, y0 + wi, ux - (float)x0, uy - (float)y0, I, diff);
      float bp[2] = {0.0f, 0.0f}, B[2];
#pragma unroll
      for (int j = 0; j < KLT_PER_LANE; ++j) {
        bp[0] += diff[j] * Ix[j];
        bp[1] += diff[j] * Iy[j];
      }
      if (!owner) bp[0] = bp[1] = 0.0f;
      wave_sums<2>(bp, lane, B);
      const float dx = (a12 * B[1] - a22 * B[0]) / D, dy = (a12 * B[0] - a11 * B[1]) / D;
      qx += dx;
      qy += dy;
      if (dx * dx + dy * dy <= a.eps2) break;
      if (it > 0 && fabsf(dx + pdx) < 0.01f && fabsf(dy + pdy) < 0.01f) {
        qx -= dx * 0.5f;
        qy -= dy * 0.5f;
        break;
      }
      pdx = dx;
      pdy = dy;
    }
    // ---- residual at the final position (level 0 only) --------------------------------------------------------------
    if (l == 0 && tracked) {
      const float ux = qx - KLT_HALF, uy = qy - KLT_HALF;
      int x0, y0;
      if (!corner_ok(ux, w, x0) || !corner_ok(uy, h, y0)) {
        tracked = false;
      } else {
        float diff[KLT_PER_LANE];
        sample_diff(lc, w, h, pitch, x0 + wj, y0 + wi, ux - (float)x0, uy - (float)y0, I, diff);
        float ep[1] = {0.0f}, E[1];
#pragma unroll
        for (int j = 0; j < KLT_PER_LANE; ++j) ep[0] += fabsf(diff[j]);
        if (!owner) ep[0] = 0.0f;
        wave_sums<1>(ep, lane, E);
        err = E[0] / (float)(KLT_WIN * KLT_WIN);
      }
    }
  }
  if (lane == 0) {
    a.px_cur[2 * (size_t)item] = qx;
    a.px_cur[2 * (size_t)item + 1] = qy;
    a.status[item] = tracked ? 1 : 0;
    a.error[item] = tracked ? err : 0.0f;
  }
}

#pragma clang fp contract(off)
// ---- trackKlt :163-164 and addSecondFrame :48-53 for one pair per workgroup ------------------------------------------
constexpr int KLT_MAX_PTS = 1024;

struct KltSumArgs {
  Cam cam;
  int n_pts;
  const float* px_ref;
  const float* px_cur;
  const uint8_t* status;
  double* f_cur;        // [n_pairs][n_pts][3]
  double* disparity;    // [n_pairs][n_pts]
  int32_t* n_tracked;   // [n_pairs]
  double* median;       // [n_pairs]
};

__global__ void __launch_bounds__(256) klt_summarize_kernel(const KltSumArgs a) {
  __shared__ double s_d[KLT_MAX_PTS];
  __shared__ uint8_t s_on[KLT_MAX_PTS];
  __shared__ int s_n;
  const int pair = (int)blockIdx.x, t = (int)threadIdx.x;
  const size_t base = (size_t)pair * a.n_pts;
  if (t == 0) s_n = 0;
  __syncthreads();
  for (int i = t; i < a.n_pts; i += 256) {
    const bool on = a.status[base + i] != 0;
    double f[3] = {0.0, 0.0, 0.0}, d = 0.0;
    if (on) {
      const float cx = a.px_cur[2 * (base + i)], cy = a.px_cur[2 * (base + i) + 1];
      cam2world(a.cam, (double)cx, (double)cy, f);  // frame_cur->c2f(px_cur.x, px_cur.y)
      // Vector2d(px_ref.x - px_cur.x, px_ref.y - px_cur.y).norm(): float differences, f64 norm
      const double ex = (double)(a.px_ref[2 * (base + i)] - cx), ey = (double)(a.px_ref[2 * (base + i) + 1] - cy);
      d = sqrt(ex * ex + ey * ey);
      atomicAdd(&s_n, 1);
    }
    a.f_cur[3 * (base + i)] = f[0];
    a.f_cur[3 * (base + i) + 1] = f[1];
    a.f_cur[3 * (base + i) + 2] = f[2];
    a.disparity[base + i] = d;
    s_d[i] = d;
    s_on[i] = on ? 1 : 0;
  }
  __syncthreads();
  const int n = s_n;
  if (t == 0) {
    a.n_tracked[pair] = n;
    if (n == 0) a.median[pair] = 0.0;
  }
  // vk::getMedian: nth_element at n / 2 -- the value of that rank among the tracked points
  block_rank_select<256>(s_d, a.n_pts, n / 2, t, [&](int j) { return s_on[j] != 0; }, &a.median[pair]);
}

}  // namespace

extern "C" {

int svo_hip_klt_params_default(svo_hip_klt_params* out) {
  if (!out) return SVO_HIP_EINVAL;
  out->win_size = 30;   // klt_win_size, initialization.cpp:136
  out->max_level = 4;   // :147
  out->max_iter = 30;   // klt_max_iter, :137
  out->eps = 0.001f;    // klt_eps, :138
  out->min_eig_threshold = 1e-4f;  // calcOpticalFlowPyrLK's default minEigThreshold
  return SVO_HIP_OK;
}

int svo_hip_klt_track(const svo_hip_pyr_layout* L, const uint8_t* d_store, int n_pairs, const int32_t* d_ref_slot,
                      const int32_t* d_cur_slot, int n_pts, const float* d_px_ref, float* d_px_cur, uint8_t* d_status,
                      float* d_error, const svo_hip_klt_params* params, void* stream) {
  if (!layout_ok(L) || !params || n_pairs < 0 || n_pts < 0) return SVO_HIP_EINVAL;
  if (params->max_level < 0 || params->max_level >= L->n_levels || params->max_iter < 0 || !(params->eps >= 0.0f) ||
      !(params->min_eig_threshold >= 0.0f) || params->win_size < 1)
    return SVO_HIP_EINVAL;
  if (params->win_size != KLT_WIN || n_pts > KLT_MAX_PTS) return SVO_HIP_ERANGE;
  if ((int64_t)n_pairs * n_pts == 0) return SVO_HIP_OK;
  if ((int64_t)n_pairs * n_pts > 0x7fffffff) return SVO_HIP_ERANGE;
  if (!d_store || !d_ref_slot || !d_cur_slot || !d_px_ref || !d_px_cur || !d_status || !d_error) return SVO_HIP_EINVAL;
  KltArgs a;
  a.L = *L;
  a.store = d_store;
  a.ref_slot = d_ref_slot; a.cur_slot = d_cur_slot;
  a.n_pts = n_pts;
  a.px_ref = d_px_ref; a.px_cur = d_px_cur; a.status = d_status; a.error = d_error;
  a.max_level = params->max_level; a.max_iter = params->max_iter;
  a.eps2 = params->eps * params->eps;
  a.min_eig_threshold = params->min_eig_threshold;
  hipLaunchKernelGGL(klt_track_kernel, dim3((unsigned)(n_pairs * n_pts)), dim3(64), 0, static_cast<hipStream_t>(stream), a);
  return check_launch();
}

int svo_hip_klt_summarize(const svo_hip_camera* cam, int n_pairs, int n_pts, const float* d_px_ref, const float* d_px_cur,
                          const uint8_t* d_status, double* d_f_cur, double* d_disparity, int32_t* d_n_tracked,
                          double* d_median_disparity, void* stream) {
  if (!cam || !cam_model_ok(cam) || n_pairs < 0 || n_pts < 0) return SVO_HIP_EINVAL;
  if (n_pts > KLT_MAX_PTS) return SVO_HIP_ERANGE;
  if (n_pairs == 0) return SVO_HIP_OK;
  if (!d_n_tracked || !d_median_disparity) return SVO_HIP_EINVAL;
  if (n_pts > 0 && (!d_px_ref || !d_px_cur || !d_status || !d_f_cur || !d_disparity)) return SVO_HIP_EINVAL;
  KltSumArgs a;
  a.cam = make_cam(cam);
  a.n_pts = n_pts;
  a.px_ref = d_px_ref; a.px_cur = d_px_cur; a.status = d_status;
  a.f_cur = d_f_cur; a.disparity = d_disparity; a.n_tracked = d_n_tracked; a.median = d_median_disparity;
  hipLaunchKernelGGL(klt_summarize_kernel, dim3((unsigned)n_pairs), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return check_launch();
}

}  // extern "C"
