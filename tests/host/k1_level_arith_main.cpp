// TEST INFRASTRUCTURE: a stand-alone program (its own main) for the per-level arithmetic of K1 that csrc/sia_common.h holds,
// compiled for the host through hip_emu.h (tests/test_k1_level_arith_host.py builds it plain and with
// -fsanitize=address,undefined):
//   (a) sia_patch_hessian<double> and <float> -- the factored H_p = [a b] S [a b]' -- against the written-out triple product
//       Sxx a_i a_j + Sxy (a_i b_j + b_i a_j) + Syy b_i b_j evaluated in long double: every entry within
//       16 x 2^-53 (2^-24) x the sum of the absolute values of its four terms.  a[1] and b[0] are handed over as NaN: the
//       helper must not read them.
//   (b) sia_ref_tile_packed -- the template of a level sampled two columns per instruction, the gradient sums without their
//       factor 0.5 -- against the scalar formulas the kernel had before (sia_bilerp per sample, dx = 0.5f * ..., the sums in
//       the order y outer, x inner), BITWISE: the 32 tile floats in the order of the LDS tile, and Sxx, Sxy, Syy.
//   (c) the pieces both K1 kernels call, BITWISE against the formulas the kernels held written out before: the tile stores
//       (plain and packed order) and the plain load on random tiles whose four unused corners are NaN; sia_jac_rows and
//       sia_jres_partials in float and double (10 000 random patches, m == false, gmask == 0, a patch on the optical axis);
//       sia_project<false> against the pinhole formula and sia_project<true> (radtan, atan) against the
//       block sia_kernel keeps written out; sia_weights at the sub-pixel positions 0 and 1 - 2^-22.
// Exits 0, the last line "ok", when everything holds.
#include "hip_emu.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "sia_common.h"

using namespace svo_sia;

namespace {

int g_fail = 0;

// ---- (a) ----------------------------------------------------------------------------------------------------------
template <typename T>
void check_hessian(double xn_, double yn_, double zi_, double fl_, double sxx_, double sxy_, double syy_, const char* what) {
  const T xn = (T)xn_, yn = (T)yn_, zi = (T)zi_, fl = (T)fl_, sxx = (T)sxx_, sxy = (T)sxy_, syy = (T)syy_;
  const T one = 1, nan = std::numeric_limits<T>::quiet_NaN();
  // the rows as the kernels form them; the two structural zeros are poisoned for the helper
  T a[6] = {-zi * fl, nan, xn * zi * fl, xn * yn * fl, -(one + xn * xn) * fl, yn * fl};
  T b[6] = {nan, -zi * fl, yn * zi * fl, (one + yn * yn) * fl, -xn * yn * fl, -xn * fl};
  T hp[21];
  sia_patch_hessian<T>(a, b, sxx, sxy, syy, hp);
  a[1] = 0;
  b[0] = 0;
  const long double eps = std::ldexp(1.0L, std::numeric_limits<T>::digits == 53 ? -53 : -24);
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) {
      const long double t1 = (long double)sxx * a[i] * a[j], t2 = (long double)sxy * a[i] * b[j];
      const long double t3 = (long double)sxy * b[i] * a[j], t4 = (long double)syy * b[i] * b[j];
      const long double want = t1 + t2 + t3 + t4;
      const long double bound = 16.0L * eps * (fabsl(t1) + fabsl(t2) + fabsl(t3) + fabsl(t4));
      const long double got = (long double)hp[sym6(i, j)];
      if (!(fabsl(got - want) <= bound)) {
        if (g_fail++ < 10)
          std::printf("%s: H(%d,%d) = %.17Lg, triple product %.17Lg, bound %.3Lg (xn %g yn %g zi %g fl %g S %g %g %g)\n", what, i, j, got,
                      want, bound, xn_, yn_, zi_, fl_, sxx_, sxy_, syy_);
      }
    }
}

int run_hessian(std::mt19937_64& rng) {
  std::uniform_real_distribution<double> u01(0.0, 1.0);
  const double fx = 315.5;
  int n = 0;
  for (int k = 0; k < 10000; ++k, ++n) {
    const double xn = -1.5 + 3.0 * u01(rng), yn = -1.5 + 3.0 * u01(rng), zi = 0.05 + 4.95 * u01(rng);
    const double fl = fx * std::ldexp(1.0, -(k % 5));
    // sums of 16 squared gradients of 8-bit images: up to 16 x 127.5^2
    const double sxx = 2.6e5 * u01(rng) * u01(rng), syy = 2.6e5 * u01(rng) * u01(rng);
    const double sxy = (2.0 * u01(rng) - 1.0) * std::sqrt(sxx * syy);
    check_hessian<double>(xn, yn, zi, fl, sxx, sxy, syy, "f64");
    check_hessian<float>(xn, yn, zi, fl, sxx, sxy, syy, "f32");
  }
  for (int l = 0; l < 5; ++l, n += 2) {
    const double fl = fx * std::ldexp(1.0, -l);
    check_hessian<double>(0.3, -0.7, 0.5, fl, 0.0, 0.0, 0.0, "f64, S = 0");
    check_hessian<float>(0.3, -0.7, 0.5, fl, 0.0, 0.0, 0.0, "f32, S = 0");
    check_hessian<double>(0.0, 0.0, 0.8, fl, 1234.5, -321.0, 987.25, "f64, xn = yn = 0");
    check_hessian<float>(0.0, 0.0, 0.8, fl, 1234.5, -321.0, 987.25, "f32, xn = yn = 0");
  }
  return n;
}

// ---- (b) ----------------------------------------------------------------------------------------------------------
// win[r][c]: the 7 x 7 bytes; rbo: where the window starts in its 12-byte runs; pad: what the other bytes of the runs hold
void check_tile(const uint8_t win[7][7], uint32_t rbo, uint8_t pad, float su, float sv, const char* what) {
  uint32_t rw[7][3];
  for (int r = 0; r < 7; ++r) {
    uint8_t run[12];
    std::memset(run, pad, sizeof run);
    for (int c = 0; c < 7; ++c) run[rbo + c] = win[r][c];
    std::memcpy(rw[r], run, 12);
  }
  float4 q[8];
  float S[3] = {-1.f, -1.f, -1.f};
  sia_ref_tile_packed(rw, rbo, su, sv, [&](int k, float4 v) { q[k] = v; }, S[0], S[1], S[2]);
  // the scalar formulas
  const float wtl = (1.f - su) * (1.f - sv), wtr = su * (1.f - sv), wbl = (1.f - su) * sv, wbr = su * sv;
  float W[7][7], Bt[6][6];
  for (int r = 0; r < 7; ++r)
    for (int c = 0; c < 7; ++c) W[r][c] = (float)win[r][c];
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) Bt[r][c] = sia_bilerp(wtl, wtr, wbl, wbr, W[r][c], W[r][c + 1], W[r + 1][c], W[r + 1][c + 1]);
  float R[3] = {0.f, 0.f, 0.f};
  for (int y = 0; y < 4; ++y)
    for (int x = 0; x < 4; ++x) {
      const float dx = 0.5f * (Bt[y + 1][x + 2] - Bt[y + 1][x]);
      const float dy = 0.5f * (Bt[y + 2][x + 1] - Bt[y][x + 1]);
      R[0] += dx * dx;
      R[1] += dx * dy;
      R[2] += dy * dy;
    }
  const float4 want[8] = {
      make_float4(Bt[0][1], Bt[0][3], Bt[0][2], Bt[0][4]), make_float4(Bt[1][0], Bt[1][2], Bt[1][1], Bt[1][3]),
      make_float4(Bt[1][4], Bt[1][5], Bt[2][0], Bt[2][2]), make_float4(Bt[2][1], Bt[2][3], Bt[2][4], Bt[2][5]),
      make_float4(Bt[3][0], Bt[3][2], Bt[3][1], Bt[3][3]), make_float4(Bt[3][4], Bt[3][5], Bt[4][0], Bt[4][2]),
      make_float4(Bt[4][1], Bt[4][3], Bt[4][4], Bt[4][5]), make_float4(Bt[5][1], Bt[5][3], Bt[5][2], Bt[5][4])};
  bool same = true;
  for (int k = 0; k < 8; ++k) {
    const float g[4] = {q[k].x, q[k].y, q[k].z, q[k].w}, w[4] = {want[k].x, want[k].y, want[k].z, want[k].w};
    same = same && std::memcmp(g, w, sizeof g) == 0;
  }
  const bool sums = std::memcmp(S, R, sizeof S) == 0;
  if (!same || !sums) {
    if (g_fail++ < 10)
      std::printf("%s (rbo %u, su %.9g, sv %.9g): tile %s, sums %.9g %.9g %.9g against %.9g %.9g %.9g\n", what, rbo, su, sv,
                  same ? "same" : "DIFFERENT", S[0], S[1], S[2], R[0], R[1], R[2]);
  }
}

int run_tiles(std::mt19937_64& rng) {
  const float step = std::ldexp(1.f, -22);  // u >= 3: the sub-pixel positions are multiples of 2^-22
  const float edge[3] = {0.f, 1.f - step, 0.5f};
  uint8_t win[7][7];
  int n = 0;
  for (int k = 0; k < 10000; ++k, ++n) {
    for (auto& row : win)
      for (auto& v : row) v = (uint8_t)(rng() & 0xff);
    const float su = (float)(rng() & 0x3fffff) * step, sv = (float)(rng() & 0x3fffff) * step;
    check_tile(win, (uint32_t)(rng() % 6), (uint8_t)(rng() & 0xff), su, sv, "random window");
  }
  // su, sv at the ends of their range, on random, constant and checkerboard windows
  for (int kind = 0; kind < 6; ++kind)
    for (int iu = 0; iu < 3; ++iu)
      for (int iv = 0; iv < 3; ++iv)
        for (uint32_t rbo = 0; rbo < 6; ++rbo, ++n) {
          for (int r = 0; r < 7; ++r)
            for (int c = 0; c < 7; ++c)
              win[r][c] = kind == 0 ? (uint8_t)(rng() & 0xff) : kind == 1 ? 0 : kind == 2 ? 255 : kind == 3 ? 77
                          : ((r + c + kind) & 1) ? 255 : 0;
          static const char* const names[6] = {"random, edge weights", "constant 0", "constant 255", "constant 77", "checkerboard", "checkerboard'"};
          check_tile(win, rbo, (uint8_t)(kind == 1 ? 255 : 0), edge[iu], edge[iv], names[kind]);
        }
  // random weights on the checkerboards
  for (int k = 0; k < 200; ++k, ++n) {
    for (int r = 0; r < 7; ++r)
      for (int c = 0; c < 7; ++c) win[r][c] = ((r + c + k) & 1) ? 255 : 0;
    check_tile(win, (uint32_t)(k % 6), 0, (float)(rng() & 0x3fffff) * step, (float)(rng() & 0x3fffff) * step, "checkerboard, random weights");
  }
  return n;
}

// ---- (c) ----------------------------------------------------------------------------------------------------------
template <typename T>
bool same_bits(const T* a, const T* b, int n) { return std::memcmp(a, b, sizeof(T) * n) == 0; }

void fail(const char* what, int k) {
  if (g_fail++ < 10) std::printf("(c) %s: case %d differs from the written-out formula\n", what, k);
}

int run_tile_slots(std::mt19937_64& rng) {
  const float nan = std::numeric_limits<float>::quiet_NaN();
  for (int k = 0; k < 2000; ++k) {
    float Bt[6][6];
    for (auto& row : Bt)
      for (auto& v : row) v = (float)(rng() & 0xffff) * (1.f / 256.f);
    Bt[0][0] = Bt[0][5] = Bt[5][0] = Bt[5][5] = nan;  // never stored
    float4 q[8], qp[8];
    for (int i = 0; i < 8; ++i) q[i] = qp[i] = make_float4(nan, nan, nan, nan);
    sia_tile_store(Bt, [&](int i) -> float4& { return q[i]; });
    sia_tile_store_packed(Bt, [&](int i) -> float4& { return qp[i]; });
    const float want[32] = {Bt[0][1], Bt[0][2], Bt[0][3], Bt[0][4], Bt[1][0], Bt[1][1], Bt[1][2], Bt[1][3], Bt[1][4], Bt[1][5], Bt[2][0],
                            Bt[2][1], Bt[2][2], Bt[2][3], Bt[2][4], Bt[2][5], Bt[3][0], Bt[3][1], Bt[3][2], Bt[3][3], Bt[3][4], Bt[3][5],
                            Bt[4][0], Bt[4][1], Bt[4][2], Bt[4][3], Bt[4][4], Bt[4][5], Bt[5][1], Bt[5][2], Bt[5][3], Bt[5][4]};
    const float wantp[32] = {Bt[0][1], Bt[0][3], Bt[0][2], Bt[0][4], Bt[1][0], Bt[1][2], Bt[1][1], Bt[1][3], Bt[1][4], Bt[1][5], Bt[2][0],
                             Bt[2][2], Bt[2][1], Bt[2][3], Bt[2][4], Bt[2][5], Bt[3][0], Bt[3][2], Bt[3][1], Bt[3][3], Bt[3][4], Bt[3][5],
                             Bt[4][0], Bt[4][2], Bt[4][1], Bt[4][3], Bt[4][4], Bt[4][5], Bt[5][1], Bt[5][3], Bt[5][2], Bt[5][4]};
    float got[32], gotp[32];
    for (int i = 0; i < 8; ++i) {
      const float a[4] = {q[i].x, q[i].y, q[i].z, q[i].w}, b[4] = {qp[i].x, qp[i].y, qp[i].z, qp[i].w};
      std::memcpy(got + 4 * i, a, sizeof a);
      std::memcpy(gotp + 4 * i, b, sizeof b);
    }
    if (!same_bits(got, want, 32)) fail("sia_tile_store", k);
    if (!same_bits(gotp, wantp, 32)) fail("sia_tile_store_packed", k);
    // the round trip: every stored sample comes back where it was, the corners as zero
    float Back[6][6];
    for (auto& row : Back)
      for (auto& v : row) v = nan;
    sia_tile_load([&](int i) { return q[i]; }, Back);
    float Want[6][6];
    std::memcpy(Want, Bt, sizeof Want);
    Want[0][0] = Want[0][5] = Want[5][0] = Want[5][5] = 0.f;
    if (!same_bits(&Back[0][0], &Want[0][0], 36)) fail("sia_tile_load", k);
    // ... and through the packed order: un-pairing the columns gives the plain slots
    float unp[32];
    std::memcpy(unp, gotp, sizeof unp);
    for (int i : {0, 4, 16, 28}) std::swap(unp[i + 1], unp[i + 2]);  // rows 0, 1, 3, 5: (a,c,b,d) -> (a,b,c,d)
    // q2 = r1 c4,5 | r2 c0,2   q3 = r2 c1,3,4,5   (and q5 / q6 alike): c2 and c1 change places across the two slots
    std::swap(unp[11], unp[12]);
    std::swap(unp[23], unp[24]);
    if (!same_bits(unp, want, 32)) fail("packed order, un-paired", k);
  }
  return 2000;
}

template <typename T>
void check_jacobian(double xn_, double yn_, double zi_, double fl_, double gmask_, bool m, double gx_, double gy_, float c2, int k) {
  const T xn = (T)xn_, yn = (T)yn_, zi = (T)zi_, fl = (T)fl_, gmask = (T)gmask_, gx = (T)gx_, gy = (T)gy_;
  T ja[6], jb[6], part[8];
  sia_jac_rows<T>(zi, xn, yn, fl, ja, jb);
  sia_jres_partials<T>(zi, xn, yn, fl, gmask, m, gx, gy, c2, part);
  // as the kernels held them
  const T one = 1, zero = 0;
  const T wa[6] = {-zi * fl, zero, xn * zi * fl, xn * yn * fl, -(one + xn * xn) * fl, yn * fl};
  const T wb[6] = {zero, -zi * fl, yn * zi * fl, (one + yn * yn) * fl, -xn * yn * fl, -xn * fl};
  const T gsc = (T)0.5 * fl * gmask;
  const T gxf = m ? gx * gsc : (T)0, gyf = m ? gy * gsc : (T)0;
  T wp[8];
  wp[0] = zi * gxf;
  wp[1] = zi * gyf;
  wp[2] = -zi * (xn * gxf + yn * gyf);
  wp[3] = -(xn * yn * gxf + ((T)1 + yn * yn) * gyf);
  wp[4] = ((T)1 + xn * xn) * gxf + xn * yn * gyf;
  wp[5] = xn * gyf - yn * gxf;
  wp[6] = (T)c2;
  wp[7] = m ? (T)16 : (T)0;
  if (!same_bits(ja, wa, 6) || !same_bits(jb, wb, 6)) fail(sizeof(T) == 8 ? "sia_jac_rows<double>" : "sia_jac_rows<float>", k);
  if (!same_bits(part, wp, 8)) fail(sizeof(T) == 8 ? "sia_jres_partials<double>" : "sia_jres_partials<float>", k);
}

int run_jacobians(std::mt19937_64& rng) {
  std::uniform_real_distribution<double> u01(0.0, 1.0);
  int n = 0;
  for (int k = 0; k < 10000; ++k, ++n) {
    const double xn = -1.5 + 3.0 * u01(rng), yn = -1.5 + 3.0 * u01(rng), zi = 0.05 + 4.95 * u01(rng);
    const double fl = 315.5 * std::ldexp(1.0, -(k % 5));
    const double gx = 4.0e4 * (2.0 * u01(rng) - 1.0), gy = 4.0e4 * (2.0 * u01(rng) - 1.0);
    const float c2 = (float)(1.0e6 * u01(rng));
    const bool m = (k % 7) != 0;
    const double gmask = (k % 11) != 0 ? 1.0 : 0.0;
    check_jacobian<double>(xn, yn, zi, fl, gmask, m, gx, gy, c2, k);
    check_jacobian<float>(xn, yn, zi, fl, gmask, m, gx, gy, c2, k);
  }
  for (int mm = 0; mm < 2; ++mm)
    for (int gm = 0; gm < 2; ++gm, ++n) {  // a patch on the optical axis; m == false; gmask == 0
      check_jacobian<double>(0.0, 0.0, 0.8, 157.75, (double)gm, mm != 0, -321.5, 77.25, 1234.5f, 10000 + n);
      check_jacobian<float>(0.0, 0.0, 0.8, 157.75, (double)gm, mm != 0, -321.5, 77.25, 1234.5f, 10000 + n);
    }
  return n;
}

int run_projection(std::mt19937_64& rng) {
  std::uniform_real_distribution<double> u01(0.0, 1.0);
  svo_hip_sia_params P{};
  P.fx = 315.5; P.fy = 314.25; P.cx = 376.0; P.cy = 240.5;
  P.cam_model = SVO_HIP_CAM_PINHOLE;
  for (int k = 0; k < 10000; ++k) {
    // a rotation by a small random vector, through the quaternion like the kernels' model
    double q[4] = {1.0, 0.1 * (u01(rng) - 0.5), 0.1 * (u01(rng) - 0.5), 0.1 * (u01(rng) - 0.5)}, R[9];
    const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (double& v : q) v /= qn;
    quat_to_R(q, R);
    const double tr[3] = {0.2 * (u01(rng) - 0.5), 0.2 * (u01(rng) - 0.5), 0.2 * (u01(rng) - 0.5)};
    const double Z = 0.5 + 9.5 * u01(rng), X = Z * (2.0 * u01(rng) - 1.0), Y = Z * (1.4 * u01(rng) - 0.7);
    double pu, pv;
    sia_project<false>(P, R, tr, X, Y, Z, pu, pv);
    const double xc = R[0] * X + R[1] * Y + R[2] * Z + tr[0];
    const double yc = R[3] * X + R[4] * Y + R[5] * Z + tr[1];
    const double zc = R[6] * X + R[7] * Y + R[8] * Z + tr[2];
    double izc = __builtin_amdgcn_rcp(zc);
    izc = fma(fma(-zc, izc, 1.0), izc, izc);
    izc = fma(fma(-zc, izc, 1.0), izc, izc);
    const double want[2] = {P.fx * (xc * izc) + P.cx, P.fy * (yc * izc) + P.cy}, got[2] = {pu, pv};
    if (!same_bits(got, want, 2)) fail("sia_project<false>", k);
    // sia_project<true> against the block sia_kernel keeps written out for its distorted instantiations
    for (int model : {SVO_HIP_CAM_PINHOLE_RADTAN, SVO_HIP_CAM_ATAN}) {
      svo_hip_sia_params D = P;
      D.cam_model = model;
      const double s = 0.93, radtan[5] = {-0.28, 0.07, 2e-4, 2e-5, 0.0};
      const double atan[5] = {s, 1.0 / s, 2.0 * std::tan(0.5 * s), 1.0 / (2.0 * std::tan(0.5 * s)), 0.0};
      for (int j = 0; j < 5; ++j) D.d[j] = model == SVO_HIP_CAM_ATAN ? atan[j] : radtan[j];
      sia_project<true>(D, R, tr, X, Y, Z, pu, pv);
      Cam cm;
      cm.fx = D.fx; cm.fy = D.fy; cm.cx = D.cx; cm.cy = D.cy;
      cm.width = 0; cm.height = 0;
      cm.model = D.cam_model;
      for (int j = 0; j < 5; ++j) cm.d[j] = D.d[j];
      const double uvn[2] = {xc * izc, yc * izc};
      double pxd[2];
      world2cam_uv(cm, uvn, pxd);
      const double gotd[2] = {pu, pv};
      if (!same_bits(gotd, pxd, 2)) fail(model == SVO_HIP_CAM_ATAN ? "sia_project<true>, atan" : "sia_project<true>, radtan", k);
    }
  }
  return 10000;
}

int run_weights(std::mt19937_64& rng) {
  const float step = std::ldexp(1.f, -22);
  int n = 0;
  for (int k = 0; k < 10000 + 9; ++k, ++n) {
    const float edge[3] = {0.f, 1.f - step, 0.5f};
    const float su = k < 9 ? edge[k / 3] : (float)(rng() & 0x3fffff) * step, sv = k < 9 ? edge[k % 3] : (float)(rng() & 0x3fffff) * step;
    float w[4];
    sia_weights(su, sv, w[0], w[1], w[2], w[3]);
    const float want[4] = {(1.f - su) * (1.f - sv), su * (1.f - sv), (1.f - su) * sv, su * sv};
    // the reference's form: the products in double, rounded to float (sparse_img_align.cpp:118-121)
    const double du = su, dv = sv;
    const float ref[4] = {(float)((1.0 - du) * (1.0 - dv)), (float)(du * (1.0 - dv)), (float)((1.0 - du) * dv), (float)(du * dv)};
    if (!same_bits(w, want, 4) || !same_bits(w, ref, 4)) fail("sia_weights", k);
  }
  return n;
}

}  // namespace

int main() {
  std::mt19937_64 rng(20240917);
  const int na = run_hessian(rng);
  std::printf("(a) %d patches, f64 and f32: %s\n", na, g_fail ? "FAILED" : "within 16 ulp of the sum of |terms|");
  const int fa = g_fail;
  const int nb = run_tiles(rng);
  std::printf("(b) %d windows: %s\n", nb, g_fail > fa ? "FAILED" : "tile and sums bit-identical to the scalar formulas");
  const int fb = g_fail;
  const int nt = run_tile_slots(rng), nj = run_jacobians(rng), np = run_projection(rng), nw = run_weights(rng);
  std::printf("(c) %d tiles, %d patches (f64 and f32), %d projections, %d weight pairs: %s\n", nt, nj, np, nw,
              g_fail > fb ? "FAILED" : "bit-identical to the written-out formulas");
  if (g_fail) return std::printf("%d mismatches\n", g_fail), 1;
  std::printf("ok\n");
  return 0;
}
