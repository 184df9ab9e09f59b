// examples/homography_init.cpp -- the second half of the two-view bootstrap through the C ABI of include/svo_hip.h from
// plain C++ (g++, no HIP headers, no torch, no reference headers): bearings of tracked points in two views go in; the
// robust homography, the pose, the inliers with their triangulated points, the metric-scaled T_f_w and the first map
// points come out of ONE call, svo_hip_homography_init -- what KltHomographyInit::addSecondFrame does after its gates
// (svo/src/initialization.cpp:56-98).
//
// Scene: 300 points of a plane at depth 2 with 3 % relief, seen from two cameras 0.4 apart and 1.5 degrees rotated;
// 0.3 px of noise on every pixel, every fifth point an outlier moved by up to 30 px, every seventh point lost.
//
//   g++ -std=c++11 -O2 -I include examples/homography_init.cpp -L rpg_svo_amd/lib -lsvo_hip
//       -Wl,-rpath,$PWD/rpg_svo_amd/lib -o build/homography_init   (one command line), then
//   build/homography_init [seed]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <svo_hip.h>

#define CK(call)                                                                          \
  do {                                                                                    \
    int rc_ = (call);                                                                     \
    if (rc_ < 0) { std::fprintf(stderr, "%s -> %s\n", #call, svo_hip_strerror(rc_)); return 1; } \
  } while (0)

struct Rng {  // a seeded generator of uniform numbers in [0, 1)
  unsigned s;
  explicit Rng(unsigned seed) : s(seed * 2654435761u + 12345u) {}
  double operator()() { s = s * 1664525u + 1013904223u; return (s >> 8) / 16777216.0; }
  double sym() { return 2.0 * (*this)() - 1.0; }
  double gauss() { double a = 0; for (int i = 0; i < 12; ++i) a += (*this)(); return a - 6.0; }
};

template <typename T>
static int to_device(void** d, const std::vector<T>& h, void* stream) {
  int rc = svo_hip_malloc(d, h.size() * sizeof(T));
  return rc < 0 ? rc : svo_hip_memcpy_h2d(*d, h.data(), h.size() * sizeof(T), stream);
}

int main(int argc, char** argv) {
  const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 7u;
  const int W = 752, H = 480, N = 300;
  const double F = 315.5, CX = 376.0, CY = 240.0, MAP_SCALE = 1.0;
  if (svo_hip_device_count() <= 0) { std::fprintf(stderr, "no HIP device: there is no CPU fallback\n"); return 2; }
  CK(svo_hip_set_device(0));

  // the true motion: 1.5 degrees about a tilted axis, 0.4 sideways and a little forward
  const double ang = 1.5 * 3.14159265358979323846 / 180.0, ax[3] = {0.36, 0.80, 0.48};
  const double c = std::cos(ang), s = std::sin(ang);
  double R[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[3 * i + j] = (i == j ? c : 0.0) + (1 - c) * ax[i] * ax[j];
  R[1] -= s * ax[2]; R[2] += s * ax[1]; R[3] += s * ax[2]; R[5] -= s * ax[0]; R[6] -= s * ax[1]; R[7] += s * ax[0];
  const double t[3] = {0.37, -0.11, 0.10};

  Rng rng(seed);
  std::vector<double> f_ref((size_t)N * 3), f_cur((size_t)N * 3), T_ref_w = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  std::vector<float> px_ref((size_t)N * 2), px_cur((size_t)N * 2);
  std::vector<uint8_t> status(N), good(N);
  const double nrm[3] = {0.05, -0.08, 0.9955};
  for (int i = 0; i < N; ++i) {
    double pr[2] = {15.0 + rng() * (W - 30.0), 15.0 + rng() * (H - 30.0)};
    const double ray[3] = {(pr[0] - CX) / F, (pr[1] - CY) / F, 1.0};
    const double depth = 2.0 * nrm[2] / (ray[0] * nrm[0] + ray[1] * nrm[1] + ray[2] * nrm[2]) * (1.0 + 0.03 * rng.sym());
    const double X[3] = {ray[0] * depth, ray[1] * depth, ray[2] * depth};
    double Y[3];
    for (int k = 0; k < 3; ++k) Y[k] = R[3 * k] * X[0] + R[3 * k + 1] * X[1] + R[3 * k + 2] * X[2] + t[k];
    double pc[2] = {F * Y[0] / Y[2] + CX, F * Y[1] / Y[2] + CY};
    for (int k = 0; k < 2; ++k) { pr[k] += 0.3 * rng.gauss(); pc[k] += 0.3 * rng.gauss(); }
    good[i] = i % 5 != 0;
    if (!good[i]) { pc[0] += 30.0 * rng.sym(); pc[1] += 30.0 * rng.sym(); }
    status[i] = i % 7 != 3;
    const double* px[2] = {pr, pc};
    double* f[2] = {&f_ref[3 * (size_t)i], &f_cur[3 * (size_t)i]};
    for (int v = 0; v < 2; ++v) {
      const double b[3] = {(px[v][0] - CX) / F, (px[v][1] - CY) / F, 1.0};
      const double n = std::sqrt(b[0] * b[0] + b[1] * b[1] + 1.0);
      for (int k = 0; k < 3; ++k) f[v][k] = b[k] / n;
    }
    px_ref[2 * i] = (float)pr[0]; px_ref[2 * i + 1] = (float)pr[1];
    px_cur[2 * i] = (float)pc[0]; px_cur[2 * i + 1] = (float)pc[1];
  }

  void* stream = NULL;
  CK(svo_hip_stream_create(&stream));
  void *d_f_ref, *d_f_cur, *d_status, *d_px_ref, *d_px_cur, *d_T;
  CK(to_device(&d_f_ref, f_ref, stream)); CK(to_device(&d_f_cur, f_cur, stream)); CK(to_device(&d_status, status, stream));
  CK(to_device(&d_px_ref, px_ref, stream)); CK(to_device(&d_px_cur, px_cur, stream)); CK(to_device(&d_T, T_ref_w, stream));
  // the outputs: one allocation, carved up in the order of svo_hip_homography_out
  const size_t n = (size_t)N;
  const size_t bytes[16] = {9 * 8, 4, 4, n, 12 * 8, 4, 4, n * 24, n, 4, 8, 8, 12 * 8, n * 24, n, 4};
  size_t off[17] = {0};
  for (int k = 0; k < 16; ++k) off[k + 1] = (off[k] + bytes[k] + 15) / 16 * 16;
  void* d_out = NULL;
  CK(svo_hip_malloc(&d_out, off[16]));
  char* base = (char*)d_out;
  svo_hip_homography_out o;
  o.d_H = (double*)(base + off[0]); o.d_best_hypothesis = (int32_t*)(base + off[1]); o.d_n_inliers_H = (int32_t*)(base + off[2]);
  o.d_inlier_H = (uint8_t*)(base + off[3]); o.d_T_cur_from_ref = (double*)(base + off[4]); o.d_ambiguous = (int32_t*)(base + off[5]);
  o.d_status = (int32_t*)(base + off[6]); o.d_xyz_in_cur = (double*)(base + off[7]); o.d_inlier = (uint8_t*)(base + off[8]);
  o.d_n_inliers = (int32_t*)(base + off[9]); o.d_depth_median = (double*)(base + off[10]); o.d_scale = (double*)(base + off[11]);
  o.d_T_cur_w = (double*)(base + off[12]); o.d_point_w = (double*)(base + off[13]); o.d_point_ok = (uint8_t*)(base + off[14]);
  o.d_result = (int32_t*)(base + off[15]);

  svo_hip_camera cam;
  CK(svo_hip_camera_pinhole(W, H, F, F, CX, CY, 0, 0, 0, 0, 0, &cam));
  svo_hip_homography_params P;
  CK(svo_hip_homography_params_default(&P));
  P.map_scale = MAP_SCALE;
  CK(svo_hip_homography_init(&cam, 1, N, (const double*)d_f_ref, (const double*)d_f_cur, (const uint8_t*)d_status, (const float*)d_px_ref,
                             (const float*)d_px_cur, (const double*)d_T, &P, &o, stream));

  std::vector<char> host(off[16]);
  CK(svo_hip_memcpy_d2h(host.data(), d_out, off[16], stream));
  CK(svo_hip_stream_sync(stream));
  const double* T = (const double*)(host.data() + off[4]);
  const double* Tw = (const double*)(host.data() + off[12]);
  const double* pw = (const double*)(host.data() + off[13]);
  const uint8_t* inlier = (const uint8_t*)(host.data() + off[8]);
  const uint8_t* point_ok = (const uint8_t*)(host.data() + off[14]);
  const int best = *(const int32_t*)(host.data() + off[1]), n_in_H = *(const int32_t*)(host.data() + off[2]);
  const int ambiguous = *(const int32_t*)(host.data() + off[5]), hstatus = *(const int32_t*)(host.data() + off[6]);
  const int n_in = *(const int32_t*)(host.data() + off[9]), result = *(const int32_t*)(host.data() + off[15]);
  const double scale = *(const double*)(host.data() + off[11]);

  double tr = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) tr += T[3 * i + j] * R[3 * i + j];
  const double rot_err = std::acos(std::max(-1.0, std::min(1.0, (tr - 1.0) / 2.0)));
  const double tn = std::sqrt(T[9] * T[9] + T[10] * T[10] + T[11] * T[11]), t0 = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
  const double dir_err = std::acos(std::max(-1.0, std::min(1.0, (T[9] * t[0] + T[10] * t[1] + T[11] * t[2]) / (tn * t0))));
  std::vector<double> depth;
  int n_good_in = 0, n_tracked_good = 0, n_ok = 0, bad_in = 0;
  for (int i = 0; i < N; ++i) {
    if (status[i] && good[i]) ++n_tracked_good;
    if (!inlier[i]) continue;
    if (!status[i]) ++bad_in;
    if (good[i]) ++n_good_in;
    n_ok += point_ok[i];
    depth.push_back(Tw[6] * pw[3 * i] + Tw[7] * pw[3 * i + 1] + Tw[8] * pw[3 * i + 2] + Tw[11]);
  }
  std::sort(depth.begin(), depth.end());
  const double median = depth.empty() ? 0.0 : depth[depth.size() / 2];
  std::printf("hypothesis %d of %d won with %d H-inliers; status %d, result %d, ambiguous %d; %d inliers (%d of the %d tracked true matches), "
              "%d map points; rotation off by %.2e rad, translation direction by %.2e rad; scale %.4f, median depth of the map %.12f\n",
              best, (int)P.n_hypotheses, n_in_H, hstatus, result, ambiguous, n_in, n_good_in, n_tracked_good, n_ok, rot_err, dir_err, scale, median);
  for (void* p : {d_f_ref, d_f_cur, d_status, d_px_ref, d_px_cur, d_T, d_out}) svo_hip_free(p);
  svo_hip_stream_destroy(stream);
  bool ok = result == SVO_HIP_INIT_SUCCESS && hstatus == SVO_HIP_HOMOGRAPHY_OK && bad_in == 0 && n_in >= P.min_inliers &&
            n_good_in >= n_tracked_good * 9 / 10 && std::fabs(median - MAP_SCALE) <= 1e-9 * MAP_SCALE;
  if (!ambiguous) ok = ok && rot_err <= 2e-2 && dir_err <= 0.1;  // (an ambiguous plane may resolve to its twin: DESIGN.md K9)
  if (!ok) { std::fprintf(stderr, "FAILED\n"); return 1; }
  std::puts("OK");
  return 0;
}
