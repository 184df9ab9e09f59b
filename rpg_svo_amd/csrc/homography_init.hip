// homography_init.hip -- K9: the second half of the two-view bootstrap on the device.
//
// Replaces what KltHomographyInit::addSecondFrame does after its gates (svo/src/initialization.cpp:56-98, 171-195:
// vk::Homography with cv::findHomography(RANSAC) and the Faugeras-Lustman decomposition, vk::computeInliers with
// triangulateFeatureNonLin, the initMinInliers decision, the scale fix and the first map points).  include/svo_hip.h
// states the algorithm step by step; tests/homography_checker.py restates it in numpy f64.
//
//   homography_init_kernel  one workgroup of 256 work-items per pair.  The tracked points are compacted into LDS as
//                           (u_ref, v_ref, u_cur, v_cur) f64 (at most 1024 x 32 B).  Work-item t owns the hypotheses
//                           k = t, t + 256, ..: four hashed picks, the four-point homography in registers, then a walk
//                           over the points as LDS broadcast reads (every lane reads the same address).  The arg-max
//                           is one integer atomicMax on a packed (score, -k) key.  Sums over points (the normal
//                           equations of a refinement step, the candidate scores, the Sampson sums) are per-lane
//                           partials in rank order, wave_reduce.h's exchange tree, and the four wave totals through
//                           LDS in a fixed order.  The small serial pieces (LDL', the 3 x 3 SVD, the eight candidates)
//                           run redundantly in every lane on workgroup-uniform values, so every branch that encloses a
//                           barrier or an exchange is taken by the whole workgroup.  Triangulation and the map
//                           points are one lane per point.
#pragma clang fp contract(off)
#include "block_select.h"
#include "capi_common.h"
#include "track_math.h"
#include "wave_reduce.h"

using namespace svo_capi;
using namespace svo_dev;

namespace {

constexpr int HI_MAX_PTS = 1024;
constexpr int HI_THREADS = 256;
constexpr int HI_MAX_HYP = 4096;
constexpr int HI_SVD_SWEEPS = 10;
constexpr double HI_COLLINEAR = 1e-10;
constexpr double HI_GAP = 1e-9;

struct HomArgs {
  Cam cam;
  int n_pts;
  const double* f_ref;
  const double* f_cur;
  const uint8_t* status;
  const float* px_ref;
  const float* px_cur;
  const double* T_ref_w;
  svo_hip_homography_params p;
  svo_hip_homography_out o;
};

__device__ __forceinline__ bool is_fin(double x) { return __builtin_isfinite(x); }

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ void cross3(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// rows of adj([p1 p2 p3]), lambda = adj p4, det; false when three of the four points are collinear
__device__ __forceinline__ bool basis(const double p[4][3], double adj[3][3], double lam[3]) {
  cross3(p[1], p[2], adj[0]);
  cross3(p[2], p[0], adj[1]);
  cross3(p[0], p[1], adj[2]);
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) q += dot3(p[i], p[i]);
  const double det = dot3(adj[2], p[2]);
  bool ok = fabs(det) >= HI_COLLINEAR * q;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    lam[i] = dot3(adj[i], p[3]);
    ok = ok && fabs(lam[i]) >= HI_COLLINEAR * q;
  }
  return ok;
}

// hypothesis k of the pair whose compacted points are s_uv[0 .. m-1]; false when it is rejected
__device__ __forceinline__ bool hypothesis(const double* s_uv, int m, uint32_t seed_mix, int k, double H[9]) {
  int pick[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t h = fmix32(seed_mix ^ (4u * (uint32_t)k + (uint32_t)j));
    int r = (int)(uint32_t)(((uint64_t)h * (uint64_t)(uint32_t)(m - j)) >> 32);
    // past the earlier picks in ascending order: count them off smallest first
    int lo = -1;
#pragma unroll
    for (int a = 0; a < j; ++a) {
      int nxt = 0x7fffffff;  // the smallest earlier pick above lo
#pragma unroll
      for (int b = 0; b < j; ++b) nxt = (pick[b] > lo && pick[b] < nxt) ? pick[b] : nxt;
      r += (r >= nxt) ? 1 : 0;
      lo = nxt;
    }
    pick[j] = r;
  }
  double p[4][3], q[4][3];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    p[j][0] = s_uv[4 * pick[j]]; p[j][1] = s_uv[4 * pick[j] + 1]; p[j][2] = 1.0;
    q[j][0] = s_uv[4 * pick[j] + 2]; q[j][1] = s_uv[4 * pick[j] + 3]; q[j][2] = 1.0;
  }
  double adjM[3][3], lam[3], adjN[3][3], mu[3];
  bool ok = basis(p, adjM, lam);
  ok = basis(q, adjN, mu) && ok;
  const double c[3] = {mu[0] * (lam[1] * lam[2]), mu[1] * (lam[0] * lam[2]), mu[2] * (lam[0] * lam[1])};
  double G[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int col = 0; col < 3; ++col)
      G[3 * r + col] = (q[0][r] * c[0]) * adjM[0][col] + (q[1][r] * c[1]) * adjM[1][col] + (q[2][r] * c[2]) * adjM[2][col];
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    H[e] = G[e] / G[8];
    ok = ok && is_fin(H[e]);
  }
  return ok;
}

// the hypothesis scores are counts behind a threshold, not bits of a sum: multiply-adds may fuse here
#pragma clang fp contract(fast)
__device__ __forceinline__ double transfer_err2(const double H[9], double u, double v, double uc, double vc) {
  const double X = H[0] * u + H[1] * v + H[2], Y = H[3] * u + H[4] * v + H[5], W = H[6] * u + H[7] * v + H[8];
  const double iw = 1.0 / W;
  const double dx = uc - X * iw, dy = vc - Y * iw;
  return dx * dx + dy * dy;
}
__device__ __forceinline__ int score_hypothesis(const double* s_uv, int m, const double H[9], double thr2) {
  int n = 0;
  for (int j = 0; j < m; ++j) n += transfer_err2(H, s_uv[4 * j], s_uv[4 * j + 1], s_uv[4 * j + 2], s_uv[4 * j + 3]) < thr2 ? 1 : 0;
  return n;
}
#pragma clang fp contract(off)

// workgroup totals of part[0 .. N-1] (N <= 8) on every work-item: wave tree, then ((w0 + w1) + w2) + w3
template <int N>
__device__ __forceinline__ void block_sums(const double part[N], int t, double* s_red, double out[N]) {
  double v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = k < N ? part[k] : 0.0;
  const double tot = wave_reduce8(v, t & 63);  // lanes 8g .. 8g+7 hold the wave's total of v[g]
  __syncthreads();                             // (the readers of the previous call are done)
  if ((t & 7) == 0) s_red[(t >> 6) * 8 + ((t & 63) >> 3)] = tot;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) out[k] = ((s_red[k] + s_red[8 + k]) + s_red[16 + k]) + s_red[24 + k];
}

// J'J (8 x 8, symmetric), J'r and the cost over the flagged ranks at H; 30 distinct sums in four exchanges
__device__ __forceinline__ void normal_equations(const double* s_uv, const uint8_t* s_flag, int m, const double H[9], int t,
                                                 double* s_red, double A[8][8], double b[8], double& cost) {
  double S[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) S[k] = 0.0;
  for (int j = t; j < m; j += HI_THREADS) {
    if (!s_flag[j]) continue;
    const double u = s_uv[4 * j], v = s_uv[4 * j + 1];
    const double X = H[0] * u + H[1] * v + H[2], Y = H[3] * u + H[4] * v + H[5], W = H[6] * u + H[7] * v + H[8];
    const double x = X / W, y = Y / W;
    const double rx = s_uv[4 * j + 2] - x, ry = s_uv[4 * j + 3] - y;
    const double a[3] = {u / W, v / W, 1.0 / W};
    S[0] += a[0] * a[0]; S[1] += a[0] * a[1]; S[2] += a[0] * a[2];
    S[3] += a[1] * a[1]; S[4] += a[1] * a[2]; S[5] += a[2] * a[2];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        S[6 + 2 * i + g] += (-x * a[i]) * a[g];
        S[12 + 2 * i + g] += (-y * a[i]) * a[g];
      }
    const double r2 = x * x + y * y;
    S[18] += r2 * (a[0] * a[0]); S[19] += r2 * (a[0] * a[1]); S[20] += r2 * (a[1] * a[1]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      S[21 + i] += rx * a[i];
      S[24 + i] += ry * a[i];
    }
    const double rr = -(rx * x + ry * y);
    S[27] += rr * a[0]; S[28] += rr * a[1];
    S[29] += rx * rx + ry * ry;
  }
  double T[32];
  block_sums<8>(S, t, s_red, T);
  block_sums<8>(S + 8, t, s_red, T + 8);
  block_sums<8>(S + 16, t, s_red, T + 16);
  block_sums<6>(S + 24, t, s_red, T + 24);
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) A[i][j] = 0.0;
  const int sym[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) A[i][j] = A[3 + i][3 + j] = T[sym[i][j]];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      A[i][6 + g] = A[6 + g][i] = T[6 + 2 * i + g];
      A[3 + i][6 + g] = A[6 + g][3 + i] = T[12 + 2 * i + g];
    }
  }
  A[6][6] = T[18]; A[6][7] = A[7][6] = T[19]; A[7][7] = T[20];
#pragma unroll
  for (int i = 0; i < 8; ++i) b[i] = T[21 + i];
  cost = T[29];
}

// A x = b by an unpivoted LDL'; false when the solution is not finite
__device__ __forceinline__ bool solve_ldl8(const double A[8][8], const double b[8], double x[8]) {
  double L[8][8], d[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    double dj = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) dj -= (L[j][k] * L[j][k]) * d[k];
    d[j] = dj;
#pragma unroll
    for (int i = j + 1; i < 8; ++i) {
      double s = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= (L[i][k] * L[j][k]) * d[k];
      L[i][j] = s / dj;
    }
  }
  double y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] = y[i] / d[i];
  bool ok = true;
#pragma unroll
  for (int i = 7; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 8; ++k) s -= L[k][i] * x[k];
    x[i] = s;
    ok = ok && is_fin(s);
  }
  return ok;
}

// one Jacobi rotation of the symmetric S in the (P, Q) plane, accumulated into the columns of V
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double S[3][3], double V[3][3]) {
  const double apq = S[P][Q];
  const bool on = apq != 0.0;
  const double theta = (S[Q][Q] - S[P][P]) / (2.0 * (on ? apq : 1.0));
  const double tt = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = on ? 1.0 / sqrt(tt * tt + 1.0) : 1.0, s = on ? tt * c : 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {  // S <- S G
    const double skp = S[k][P], skq = S[k][Q];
    S[k][P] = c * skp - s * skq;
    S[k][Q] = s * skp + c * skq;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {  // S <- G' S
    const double spk = S[P][k], sqk = S[Q][k];
    S[P][k] = c * spk - s * sqk;
    S[Q][k] = s * spk + c * sqk;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vkp = V[k][P], vkq = V[k][Q];
    V[k][P] = c * vkp - s * vkq;
    V[k][Q] = s * vkp + c * vkq;
  }
}

template <int P, int Q>
__device__ __forceinline__ void sort_columns(double e[3], double V[3][3]) {
  const bool sw = e[P] < e[Q];
  const double ep = e[P], eq = e[Q];
  e[P] = sw ? eq : ep;
  e[Q] = sw ? ep : eq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vp = V[k][P], vq = V[k][Q];
    V[k][P] = sw ? vq : vp;
    V[k][Q] = sw ? vp : vq;
  }
}

__device__ __forceinline__ double det3(const double M[3][3]) {
  return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
         M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
}

struct Svd3 {
  double U[3][3], V[3][3], d[3], s;
};

// H = U diag(d) V' as include/svo_hip.h forms it; false when the decomposition is degenerate
__device__ __forceinline__ bool svd3(const double H[9], Svd3& o) {
  double S[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      S[i][j] = H[i] * H[j] + H[3 + i] * H[3 + j] + H[6 + i] * H[6 + j];
      o.V[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < HI_SVD_SWEEPS; ++sweep) {
    jacobi_rotate<0, 1>(S, o.V);
    jacobi_rotate<0, 2>(S, o.V);
    jacobi_rotate<1, 2>(S, o.V);
  }
  double e[3] = {S[0][0], S[1][1], S[2][2]};
  sort_columns<0, 1>(e, o.V);
  sort_columns<0, 2>(e, o.V);
  sort_columns<1, 2>(e, o.V);
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    o.d[i] = sqrt(e[i]);
    const double a0 = fabs(o.V[0][i]), a1 = fabs(o.V[1][i]), a2 = fabs(o.V[2][i]);
    const double big = (a0 >= a1 && a0 >= a2) ? o.V[0][i] : (a1 >= a2 ? o.V[1][i] : o.V[2][i]);
    const double sg = big < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) o.V[k][i] = sg * o.V[k][i];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      o.U[k][i] = (H[3 * k] * o.V[0][i] + H[3 * k + 1] * o.V[1][i] + H[3 * k + 2] * o.V[2][i]) / o.d[i];
      ok = ok && is_fin(o.U[k][i]) && is_fin(o.V[k][i]);
    }
    ok = ok && is_fin(o.d[i]);
  }
  o.s = det3(o.U) * det3(o.V) < 0.0 ? -1.0 : 1.0;
  ok = ok && !(o.d[0] - o.d[1] < HI_GAP * o.d[1]) && !(o.d[1] - o.d[2] < HI_GAP * o.d[1]);
  return ok;
}

struct Candidate {
  double R[9], t[3], n[3], d;
};

__device__ __forceinline__ void candidate(const Svd3& f, int c, Candidate& o) {
  const double d1 = f.d[0], d2 = f.d[1], d3 = f.d[2];
  const double den = d1 * d1 - d3 * d3;
  const double x1 = sqrt((d1 * d1 - d2 * d2) / den), x3 = sqrt((d2 * d2 - d3 * d3) / den);
  const double e1 = (c & 1) ? -1.0 : 1.0, e3 = (c & 2) ? -1.0 : 1.0;
  const bool pos = c < 4;
  double Rp[3][3], tp[3];
  if (pos) {
    const double sn = (d1 - d3) * x1 * x3 * e1 * e3 / d2, cs = (d1 * (x3 * x3) + d3 * (x1 * x1)) / d2;
    Rp[0][0] = cs; Rp[0][1] = 0.0; Rp[0][2] = -sn;
    Rp[1][0] = 0.0; Rp[1][1] = 1.0; Rp[1][2] = 0.0;
    Rp[2][0] = sn; Rp[2][1] = 0.0; Rp[2][2] = cs;
    tp[0] = (d1 - d3) * (x1 * e1); tp[1] = 0.0; tp[2] = (d1 - d3) * (-x3 * e3);
    o.d = f.s * d2;
  } else {
    const double sn = (d1 + d3) * x1 * x3 * e1 * e3 / d2, cs = (d3 * (x1 * x1) - d1 * (x3 * x3)) / d2;
    Rp[0][0] = cs; Rp[0][1] = 0.0; Rp[0][2] = sn;
    Rp[1][0] = 0.0; Rp[1][1] = -1.0; Rp[1][2] = 0.0;
    Rp[2][0] = sn; Rp[2][1] = 0.0; Rp[2][2] = -cs;
    tp[0] = (d1 + d3) * (x1 * e1); tp[1] = 0.0; tp[2] = (d1 + d3) * (x3 * e3);
    o.d = -f.s * d2;
  }
  const double np[3] = {x1 * e1, 0.0, x3 * e3};
  double URp[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) URp[i][j] = f.U[i][0] * Rp[0][j] + f.U[i][1] * Rp[1][j] + f.U[i][2] * Rp[2][j];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) o.R[3 * i + j] = f.s * (URp[i][0] * f.V[j][0] + URp[i][1] * f.V[j][1] + URp[i][2] * f.V[j][2]);
    o.t[i] = f.U[i][0] * tp[0] + f.U[i][1] * tp[1] + f.U[i][2] * tp[2];
    o.n[i] = f.V[i][0] * np[0] + f.V[i][1] * np[1] + f.V[i][2] * np[2];
  }
}

// the rank of entry c in a stable descending sort of score[0 .. 7] by (score, tie)
__device__ __forceinline__ void stable_ranks(const double score[8], const int tie[8], const bool in[8], int rank[8]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    int r = 0;
#pragma unroll
    for (int o = 0; o < 8; ++o) r += (in[o] && (score[o] > score[c] || (score[o] == score[c] && tie[o] < tie[c]))) ? 1 : 0;
    rank[c] = in[c] ? r : 8;
  }
}

__device__ __forceinline__ void essential(const Candidate& c, double E[9]) {
  // [t]x R
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    E[j] = c.t[1] * c.R[6 + j] - c.t[2] * c.R[3 + j];
    E[3 + j] = c.t[2] * c.R[j] - c.t[0] * c.R[6 + j];
    E[6 + j] = c.t[0] * c.R[3 + j] - c.t[1] * c.R[j];
  }
}

__device__ __forceinline__ double sampson(const double E[9], double u, double v, double uc, double vc, double cap) {
  const double l0 = E[0] * u + E[1] * v + E[2], l1 = E[3] * u + E[4] * v + E[5], l2 = E[6] * u + E[7] * v + E[8];
  const double m0 = E[0] * uc + E[3] * vc + E[6], m1 = E[1] * uc + E[4] * vc + E[7];
  const double e = uc * l0 + vc * l1 + l2;
  const double err = (e * e) / (l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1);
  return err < cap ? err : cap;
}

__global__ void __launch_bounds__(HI_THREADS) homography_init_kernel(const HomArgs a) {
  __shared__ double s_uv[4 * HI_MAX_PTS];   // compacted (u_ref, v_ref, u_cur, v_cur)
  __shared__ double s_z[HI_MAX_PTS];        // xyz.z of the inliers, by rank
  __shared__ int s_idx[HI_MAX_PTS];         // rank -> point index
  __shared__ uint8_t s_flag[HI_MAX_PTS];    // per rank: the winner's inliers, later H-inliers, later inliers
  __shared__ double s_red[32];
  __shared__ int s_wcnt[4];
  __shared__ int s_best;
  __shared__ double s_med;
  const int pair = (int)blockIdx.x, t = (int)threadIdx.x;
  const int n_pts = a.n_pts;
  const size_t base = (size_t)pair * n_pts;
  const svo_hip_homography_out& o = a.o;

  // ---- defined zeros everywhere; the steps that are reached overwrite their own (same work-item, same address) -------
  for (int i = t; i < n_pts; i += HI_THREADS) {
    o.d_inlier_H[base + i] = 0;
    o.d_inlier[base + i] = 0;
    o.d_point_ok[base + i] = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      o.d_xyz_in_cur[3 * (base + i) + k] = 0.0;
      o.d_point_w[3 * (base + i) + k] = 0.0;
    }
  }
  if (t < 12) {
    o.d_T_cur_from_ref[12 * (size_t)pair + t] = 0.0;
    o.d_T_cur_w[12 * (size_t)pair + t] = 0.0;
  }
  if (t < 9) o.d_H[9 * (size_t)pair + t] = 0.0;
  if (t == 0) {
    o.d_best_hypothesis[pair] = -1;
    o.d_n_inliers_H[pair] = 0;
    o.d_ambiguous[pair] = 0;
    o.d_status[pair] = SVO_HIP_HOMOGRAPHY_NO_MODEL;
    o.d_n_inliers[pair] = 0;
    o.d_depth_median[pair] = 0.0;
    o.d_scale[pair] = 0.0;
    o.d_result[pair] = SVO_HIP_INIT_FAILURE;
    s_best = -1;
  }

  // ---- compaction in index order ----------------------------------------------------------------------------------------
  int m = 0;
  for (int c0 = 0; c0 < n_pts; c0 += HI_THREADS) {
    const int i = c0 + t;
    const bool on = i < n_pts && a.status[base + (i < n_pts ? i : 0)] != 0;
    const int j = block_compact_step<HI_THREADS / 64>(on, t, s_wcnt, m);
    if (on) {
      const double* fr = a.f_ref + 3 * (base + i);
      const double* fc = a.f_cur + 3 * (base + i);
      s_uv[4 * j] = fr[0] / fr[2];
      s_uv[4 * j + 1] = fr[1] / fr[2];
      s_uv[4 * j + 2] = fc[0] / fc[2];
      s_uv[4 * j + 3] = fc[1] / fc[2];
      s_idx[j] = i;
    }
  }
  __syncthreads();
  if (m < 4) return;  // NO_MODEL (workgroup-uniform)

  const double focal = fabs(a.cam.fx), focal2 = focal * focal;
  const double thr = a.p.reproj_thresh;

  // ---- 1. hypotheses ----------------------------------------------------------------------------------------------------
  const uint32_t seed_mix = fmix32(a.p.seed + 0x9e3779b9u);
  const double ransac_thr2 = 4.0 / focal2;
  int key = -1;
  for (int k = t; k < a.p.n_hypotheses; k += HI_THREADS) {
    double Hk[9];
    const bool ok = hypothesis(s_uv, m, seed_mix, k, Hk);
    const int score = score_hypothesis(s_uv, m, Hk, ransac_thr2);
    const int kk = ok ? score * HI_MAX_HYP + (HI_MAX_HYP - 1 - k) : -1;
    key = kk > key ? kk : key;
  }
  atomicMax(&s_best, key);
  __syncthreads();
  const int best_key = s_best;
  if (best_key < 0) return;  // every hypothesis rejected: NO_MODEL
  const int best = HI_MAX_HYP - 1 - (best_key % HI_MAX_HYP);
  double H[9];
  hypothesis(s_uv, m, seed_mix, best, H);
  for (int j = t; j < m; j += HI_THREADS)
    s_flag[j] = transfer_err2(H, s_uv[4 * j], s_uv[4 * j + 1], s_uv[4 * j + 2], s_uv[4 * j + 3]) < ransac_thr2 ? 1 : 0;
  __syncthreads();

  // ---- 2. refinement -----------------------------------------------------------------------------------------------------
  {
    double Ht[9], cost_good = 0.0;
#pragma unroll
    for (int e = 0; e < 9; ++e) Ht[e] = H[e];
    for (int it = 0; it <= a.p.refine_iters; ++it) {
      if (it == 0 && a.p.refine_iters == 0) break;
      double A[8][8], b[8], cost, delta[8];
      normal_equations(s_uv, s_flag, m, Ht, t, s_red, A, b, cost);
      if (it > 0 && !(cost <= cost_good)) break;
#pragma unroll
      for (int e = 0; e < 9; ++e) H[e] = Ht[e];
      cost_good = cost;
      if (it == a.p.refine_iters) break;
      if (!solve_ldl8(A, b, delta)) break;
#pragma unroll
      for (int e = 0; e < 8; ++e) Ht[e] = H[e] + delta[e];
    }
  }

  // ---- 3. inliers of H -----------------------------------------------------------------------------------------------------
  const double thr2 = thr * thr;
  double cnt[8];
  {
    double part[2] = {0.0, 0.0};
    __syncthreads();
    for (int j = t; j < m; j += HI_THREADS) {
      const double u = s_uv[4 * j], v = s_uv[4 * j + 1];
      const double W = H[6] * u + H[7] * v + H[8];
      const double x = (H[0] * u + H[1] * v + H[2]) / W, y = (H[3] * u + H[4] * v + H[5]) / W;
      const double dx = s_uv[4 * j + 2] - x, dy = s_uv[4 * j + 3] - y;
      const bool in = focal2 * (dx * dx + dy * dy) < thr2;
      s_flag[j] = in ? 1 : 0;
      o.d_inlier_H[base + s_idx[j]] = in ? 1 : 0;
      part[0] += in ? 1.0 : 0.0;
    }
    block_sums<1>(part, t, s_red, cnt);
  }
  const int n_in_H = (int)cnt[0];
  if (t == 0) {
#pragma unroll
    for (int e = 0; e < 9; ++e) o.d_H[9 * (size_t)pair + e] = H[e];  // (constant indices: the arrays stay in registers)
    o.d_best_hypothesis[pair] = best;
    o.d_n_inliers_H[pair] = n_in_H;
  }

  // ---- 4. decomposition ----------------------------------------------------------------------------------------------------
  Svd3 f;
  if (!svd3(H, f)) {
    if (t == 0) o.d_status[pair] = SVO_HIP_HOMOGRAPHY_DEGENERATE;
    return;
  }
  if (t == 0) o.d_status[pair] = SVO_HIP_HOMOGRAPHY_OK;

  // ---- 5. choice -------------------------------------------------------------------------------------------------------------
  double score1[8], score2[8];
  {
    double n8[8][3], d8[8], part[8], side[2] = {0.0, 0.0}, tot[2];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      Candidate cd;
      candidate(f, c, cd);
      n8[c][0] = cd.n[0]; n8[c][1] = cd.n[1]; n8[c][2] = cd.n[2];
      d8[c] = cd.d;
      part[c] = 0.0;
    }
    for (int j = t; j < m; j += HI_THREADS) {
      if (!s_flag[j]) continue;
      const double u = s_uv[4 * j], v = s_uv[4 * j + 1];
      const double W = H[6] * u + H[7] * v + H[8];
      side[0] += W / d8[0] > 0.0 ? 1.0 : 0.0;
      side[1] += W / d8[4] > 0.0 ? 1.0 : 0.0;
#pragma unroll
      for (int c = 0; c < 8; ++c) part[c] += (u * n8[c][0] + v * n8[c][1] + n8[c][2]) / d8[c] > 0.0 ? 1.0 : 0.0;
    }
    block_sums<2>(side, t, s_red, tot);
    block_sums<8>(part, t, s_red, score2);
#pragma unroll
    for (int c = 0; c < 8; ++c) score1[c] = c < 4 ? tot[0] : tot[1];
  }
  int first = 0, second = 0;
  {
    int tie[8], rank1[8], rank2[8];
    bool all[8], kept[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { tie[c] = c; all[c] = true; }
    stable_ranks(score1, tie, all, rank1);
#pragma unroll
    for (int c = 0; c < 8; ++c) kept[c] = rank1[c] < 4;
    stable_ranks(score2, rank1, kept, rank2);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      first = rank2[c] == 0 ? c : first;
      second = rank2[c] == 1 ? c : second;
    }
  }
  double sc_first = 0.0, sc_second = 0.0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    sc_first = c == first ? score2[c] : sc_first;
    sc_second = c == second ? score2[c] : sc_second;
  }
  Candidate win;
  candidate(f, first, win);
  int ambiguous = 0;
  if (!(sc_second / sc_first < 0.9)) {
    ambiguous = 1;
    Candidate other;
    candidate(f, second, other);
    double E0[9], E1[9], part[2] = {0.0, 0.0}, tot[2];
    essential(win, E0);
    essential(other, E1);
    const double cap = 4.0 * (thr / focal) * (thr / focal);
    for (int j = t; j < m; j += HI_THREADS) {
      part[0] += sampson(E0, s_uv[4 * j], s_uv[4 * j + 1], s_uv[4 * j + 2], s_uv[4 * j + 3], cap);
      part[1] += sampson(E1, s_uv[4 * j], s_uv[4 * j + 1], s_uv[4 * j + 2], s_uv[4 * j + 3], cap);
    }
    block_sums<2>(part, t, s_red, tot);
    if (tot[1] < tot[0]) win = other;
  }
  if (t == 0) {
#pragma unroll
    for (int e = 0; e < 9; ++e) o.d_T_cur_from_ref[12 * (size_t)pair + e] = win.R[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) o.d_T_cur_from_ref[12 * (size_t)pair + 9 + e] = win.t[e];
    o.d_ambiguous[pair] = ambiguous;
  }

  // ---- 6. computeInliers: one lane per point ------------------------------------------------------------------------------------
  __syncthreads();  // (s_flag is rewritten)
  {
    double part[1] = {0.0};
    for (int j = t; j < m; j += HI_THREADS) {
      const size_t gi = base + s_idx[j];
      const double fc[3] = {a.f_cur[3 * gi], a.f_cur[3 * gi + 1], a.f_cur[3 * gi + 2]};
      const double fr[3] = {a.f_ref[3 * gi], a.f_ref[3 * gi + 1], a.f_ref[3 * gi + 2]};
      double f2[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) f2[i] = win.R[3 * i] * fr[0] + win.R[3 * i + 1] * fr[1] + win.R[3 * i + 2] * fr[2];
      const double a00 = dot3(fc, fc), a10 = dot3(fc, f2), a01 = -a10, a11 = -dot3(f2, f2);
      const double b0 = dot3(win.t, fc), b1 = dot3(win.t, f2);
      const double det = a00 * a11 - a01 * a10;
      const double l0 = (a11 * b0 - a01 * b1) / det, l1 = (a00 * b1 - a10 * b0) / det;
      double xyz[3], back[3], dlt[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        xyz[i] = (l0 * fc[i] + (win.t[i] + l1 * f2[i])) / 2.0;
        dlt[i] = xyz[i] - win.t[i];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) back[i] = win.R[i] * dlt[0] + win.R[3 + i] * dlt[1] + win.R[6 + i] * dlt[2];
      const double ex1 = s_uv[4 * j + 2] - xyz[0] / xyz[2], ey1 = s_uv[4 * j + 3] - xyz[1] / xyz[2];
      const double ex2 = s_uv[4 * j] - back[0] / back[2], ey2 = s_uv[4 * j + 1] - back[1] / back[2];
      const double e1 = focal * sqrt(ex1 * ex1 + ey1 * ey1), e2 = focal * sqrt(ex2 * ex2 + ey2 * ey2);
      const bool in = e1 <= thr && e2 <= thr;
      s_flag[j] = in ? 1 : 0;
      s_z[j] = in ? xyz[2] : 0.0;
      o.d_inlier[gi] = in ? 1 : 0;
#pragma unroll
      for (int i = 0; i < 3; ++i) o.d_xyz_in_cur[3 * gi + i] = in ? xyz[i] : 0.0;
      part[0] += in ? 1.0 : 0.0;
    }
    block_sums<1>(part, t, s_red, cnt);
  }
  const int n_in = (int)cnt[0];
  if (t == 0) o.d_n_inliers[pair] = n_in;
  if (n_in < a.p.min_inliers || n_in == 0) return;  // FAILURE

  // ---- 7. scale and map -----------------------------------------------------------------------------------------------------------
  // vk::getMedian of the n_in > 0 inlier depths: exactly one rank matches
  block_rank_select<HI_THREADS>(s_z, m, n_in / 2, t, [&](int j) { return s_flag[j] != 0; }, &s_med);
  __syncthreads();
  const double depth_median = s_med;
  const double scale = a.p.map_scale / depth_median;
  double Rw[9], tw[3];
  {
    const double* Tr = a.T_ref_w + 12 * (size_t)pair;
    double t_cw[3], pos_ref[3], pos_cur[3], mix[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) Rw[3 * i + j] = win.R[3 * i] * Tr[j] + win.R[3 * i + 1] * Tr[3 + j] + win.R[3 * i + 2] * Tr[6 + j];
      t_cw[i] = (win.R[3 * i] * Tr[9] + win.R[3 * i + 1] * Tr[10] + win.R[3 * i + 2] * Tr[11]) + win.t[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      pos_ref[i] = -(Tr[i] * Tr[9] + Tr[3 + i] * Tr[10] + Tr[6 + i] * Tr[11]);
      pos_cur[i] = -(Rw[i] * t_cw[0] + Rw[3 + i] * t_cw[1] + Rw[6 + i] * t_cw[2]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) mix[i] = pos_ref[i] + scale * (pos_cur[i] - pos_ref[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) tw[i] = -(Rw[3 * i] * mix[0] + Rw[3 * i + 1] * mix[1] + Rw[3 * i + 2] * mix[2]);
  }
  if (t == 0) {
#pragma unroll
    for (int e = 0; e < 9; ++e) o.d_T_cur_w[12 * (size_t)pair + e] = Rw[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) o.d_T_cur_w[12 * (size_t)pair + 9 + e] = tw[e];
    o.d_depth_median[pair] = depth_median;
    o.d_scale[pair] = scale;
    o.d_result[pair] = SVO_HIP_INIT_SUCCESS;
  }
  for (int j = t; j < m; j += HI_THREADS) {
    if (!s_flag[j]) continue;
    const size_t gi = base + s_idx[j];
    const double xyz[3] = {o.d_xyz_in_cur[3 * gi], o.d_xyz_in_cur[3 * gi + 1], o.d_xyz_in_cur[3 * gi + 2]};  // this work-item's own store
    const double v[3] = {xyz[0] * scale - tw[0], xyz[1] * scale - tw[1], xyz[2] * scale - tw[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) o.d_point_w[3 * gi + i] = Rw[i] * v[0] + Rw[3 + i] * v[1] + Rw[6 + i] * v[2];
    const int cx = cast_int((double)a.px_cur[2 * gi]), cy = cast_int((double)a.px_cur[2 * gi + 1]);
    const int rx = cast_int((double)a.px_ref[2 * gi]), ry = cast_int((double)a.px_ref[2 * gi + 1]);
    o.d_point_ok[gi] = (is_in_frame(a.cam, cx, cy, 10) && is_in_frame(a.cam, rx, ry, 10) && xyz[2] > 0.0) ? 1 : 0;
  }
}

}  // namespace

extern "C" {

int svo_hip_homography_params_default(svo_hip_homography_params* out) {
  if (!out) return SVO_HIP_EINVAL;
  out->reproj_thresh = 2.0;  // Config::poseOptimThresh()
  out->map_scale = 1.0;      // Config::mapScale()
  out->min_inliers = 40;     // Config::initMinInliers()
  out->n_hypotheses = 512;
  out->refine_iters = 10;
  out->seed = 0;
  return SVO_HIP_OK;
}

int svo_hip_homography_init(const svo_hip_camera* cam, int n_pairs, int n_pts, const double* d_f_ref, const double* d_f_cur,
                            const uint8_t* d_status, const float* d_px_ref, const float* d_px_cur, const double* d_T_ref_w,
                            const svo_hip_homography_params* params, const svo_hip_homography_out* out, void* stream) {
  if (!cam || !cam_model_ok(cam) || !params || !out || n_pairs < 0 || n_pts < 0) return SVO_HIP_EINVAL;
  if (!(params->reproj_thresh > 0.0) || params->refine_iters < 0 || params->min_inliers < 0) return SVO_HIP_EINVAL;
  if (n_pts > HI_MAX_PTS || params->n_hypotheses < 1 || params->n_hypotheses > HI_MAX_HYP) return SVO_HIP_ERANGE;
  if ((int64_t)n_pairs * n_pts == 0) return SVO_HIP_OK;
  if ((int64_t)n_pairs * n_pts > 0x7fffffff) return SVO_HIP_ERANGE;
  if (!d_f_ref || !d_f_cur || !d_status || !d_px_ref || !d_px_cur || !d_T_ref_w) return SVO_HIP_EINVAL;
  if (!out->d_H || !out->d_best_hypothesis || !out->d_n_inliers_H || !out->d_inlier_H || !out->d_T_cur_from_ref ||
      !out->d_ambiguous || !out->d_status || !out->d_xyz_in_cur || !out->d_inlier || !out->d_n_inliers || !out->d_depth_median ||
      !out->d_scale || !out->d_T_cur_w || !out->d_point_w || !out->d_point_ok || !out->d_result)
    return SVO_HIP_EINVAL;
  HomArgs a;
  a.cam = make_cam(cam);
  a.n_pts = n_pts;
  a.f_ref = d_f_ref; a.f_cur = d_f_cur; a.status = d_status; a.px_ref = d_px_ref; a.px_cur = d_px_cur; a.T_ref_w = d_T_ref_w;
  a.p = *params;
  a.o = *out;
  hipLaunchKernelGGL(homography_init_kernel, dim3((unsigned)n_pairs), dim3(HI_THREADS), 0, static_cast<hipStream_t>(stream), a);
  return check_launch();
}

}  // extern "C"
