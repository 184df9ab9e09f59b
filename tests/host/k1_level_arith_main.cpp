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

}  // namespace

int main() {
  std::mt19937_64 rng(20240917);
  const int na = run_hessian(rng);
  std::printf("(a) %d patches, f64 and f32: %s\n", na, g_fail ? "FAILED" : "within 16 ulp of the sum of |terms|");
  const int fa = g_fail;
  const int nb = run_tiles(rng);
  std::printf("(b) %d windows: %s\n", nb, g_fail > fa ? "FAILED" : "tile and sums bit-identical to the scalar formulas");
  if (g_fail) return std::printf("%d mismatches\n", g_fail), 1;
  std::printf("ok\n");
  return 0;
}
