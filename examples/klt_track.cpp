// examples/klt_track.cpp -- the bootstrap's tracker through the C ABI of include/svo_hip.h from plain C++ (g++, no HIP
// headers, no torch, no reference headers): two images, their pyramids built on the device, corners on a grid tracked
// from the first into the second with svo_hip_klt_track, then bearings, disparities and their median with
// svo_hip_klt_summarize -- what initialization::trackKlt and the gates of KltHomographyInit::addSecondFrame compute.
//
// Scene: a seeded smooth texture and the same texture moved by a known sub-pixel translation.  A pure translation is
// what Lucas-Kanade models exactly, so every tracked point must come back within 0.05 px of it (50 x the tracker's
// stop threshold of 0.001 px).
//
//   g++ -std=c++11 -O2 -I include examples/klt_track.cpp -L rpg_svo_amd/lib -lsvo_hip
//       -Wl,-rpath,$PWD/rpg_svo_amd/lib -o build/klt_track   (one command line), then
//   build/klt_track [seed]
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

struct Texture {  // a sum of plane waves with seeded directions and phases: smooth, gradients everywhere
  double kx[12], ky[12], ph[12], amp[12];
  explicit Texture(unsigned seed) {
    unsigned s = seed * 2654435761u + 12345u;
    for (int k = 0; k < 12; ++k) {
      double r[3];
      for (int j = 0; j < 3; ++j) { s = s * 1664525u + 1013904223u; r[j] = (s >> 8) / 16777216.0; }
      const double wavelength = 14.0 + 50.0 * r[0], dir = 6.283185307179586 * r[1];
      kx[k] = 6.283185307179586 / wavelength * std::cos(dir);
      ky[k] = 6.283185307179586 / wavelength * std::sin(dir);
      ph[k] = 6.283185307179586 * r[2];
      amp[k] = 9.0;
    }
  }
  double operator()(double x, double y) const {
    double v = 128.0;
    for (int k = 0; k < 12; ++k) v += amp[k] * std::sin(kx[k] * x + ky[k] * y + ph[k]);
    return v;
  }
};

int main(int argc, char** argv) {
  const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 7u;
  const int W = 640, H = 480, LEVELS = 5, COLS = 16, ROWS = 12, N = COLS * ROWS;
  const double sx = 3.4, sy = -2.3;
  if (svo_hip_device_count() <= 0) { std::fprintf(stderr, "no HIP device: there is no CPU fallback\n"); return 2; }
  CK(svo_hip_set_device(0));

  const Texture texture(seed);
  std::vector<uint8_t> ref((size_t)W * H), cur((size_t)W * H);
  for (int v = 0; v < H; ++v)
    for (int u = 0; u < W; ++u) {
      ref[(size_t)v * W + u] = (uint8_t)std::lround(texture(u, v));
      cur[(size_t)v * W + u] = (uint8_t)std::lround(texture(u - sx, v - sy));  // content moved by (+sx, +sy)
    }
  svo_hip_pyr_layout L;
  CK(svo_hip_pyr_layout_init(W, H, LEVELS, &L));
  void* d_store = NULL;
  CK(svo_hip_malloc(&d_store, (size_t)svo_hip_pyr_store_bytes(&L, 2)));
  CK(svo_hip_memset(d_store, 0, (size_t)svo_hip_pyr_store_bytes(&L, 2), NULL));
  void* stream = NULL;
  CK(svo_hip_stream_create(&stream));
  CK(svo_hip_pyramid_upload_build(&L, (uint8_t*)d_store, 0, ref.data(), W, SVO_HIP_HALFSAMPLE_AUTO, NULL, stream));
  CK(svo_hip_pyramid_upload_build(&L, (uint8_t*)d_store, 1, cur.data(), W, SVO_HIP_HALFSAMPLE_AUTO, NULL, stream));

  // corners on a grid, 40 px inside; the initial flow is "no motion" (px_cur = px_ref, initialization.cpp:39)
  std::vector<float> px_ref((size_t)N * 2);
  for (int i = 0; i < N; ++i) {
    px_ref[2 * i] = 40.0f + (float)(i % COLS) * (float)(W - 80) / (float)(COLS - 1);
    px_ref[2 * i + 1] = 40.0f + (float)(i / COLS) * (float)(H - 80) / (float)(ROWS - 1);
  }
  const std::vector<uint8_t> ones(N, 1);
  const int32_t slots[2] = {0, 1};
  void *d_slots, *d_px_ref, *d_px_cur, *d_status, *d_error, *d_f, *d_disp, *d_n, *d_med;
  CK(svo_hip_malloc(&d_slots, 8)); CK(svo_hip_malloc(&d_px_ref, (size_t)N * 8)); CK(svo_hip_malloc(&d_px_cur, (size_t)N * 8));
  CK(svo_hip_malloc(&d_status, N)); CK(svo_hip_malloc(&d_error, (size_t)N * 4)); CK(svo_hip_malloc(&d_f, (size_t)N * 24));
  CK(svo_hip_malloc(&d_disp, (size_t)N * 8)); CK(svo_hip_malloc(&d_n, 4)); CK(svo_hip_malloc(&d_med, 8));
  CK(svo_hip_memcpy_h2d(d_slots, slots, 8, stream));
  CK(svo_hip_memcpy_h2d(d_px_ref, px_ref.data(), (size_t)N * 8, stream));
  CK(svo_hip_memcpy_h2d(d_px_cur, px_ref.data(), (size_t)N * 8, stream));
  CK(svo_hip_memcpy_h2d(d_status, ones.data(), N, stream));

  svo_hip_klt_params P;
  CK(svo_hip_klt_params_default(&P));
  svo_hip_camera cam;
  CK(svo_hip_camera_pinhole(W, H, 400, 400, 320, 240, 0, 0, 0, 0, 0, &cam));
  CK(svo_hip_klt_track(&L, (const uint8_t*)d_store, 1, (const int32_t*)d_slots, (const int32_t*)d_slots + 1, N, (const float*)d_px_ref,
                       (float*)d_px_cur, (uint8_t*)d_status, (float*)d_error, &P, stream));
  CK(svo_hip_klt_summarize(&cam, 1, N, (const float*)d_px_ref, (const float*)d_px_cur, (const uint8_t*)d_status, (double*)d_f,
                           (double*)d_disp, (int32_t*)d_n, (double*)d_med, stream));

  std::vector<float> px_cur((size_t)N * 2), error(N);
  std::vector<uint8_t> status(N);
  int32_t n_tracked = 0;
  double median = 0;
  CK(svo_hip_memcpy_d2h(px_cur.data(), d_px_cur, (size_t)N * 8, stream));
  CK(svo_hip_memcpy_d2h(error.data(), d_error, (size_t)N * 4, stream));
  CK(svo_hip_memcpy_d2h(status.data(), d_status, N, stream));
  CK(svo_hip_memcpy_d2h(&n_tracked, d_n, 4, stream));
  CK(svo_hip_memcpy_d2h(&median, d_med, 8, stream));
  CK(svo_hip_stream_sync(stream));

  double worst = 0, mx = 0, my = 0, worst_residual = 0;
  int n = 0;
  for (int i = 0; i < N; ++i) {
    if (!status[i]) continue;
    const double dx = px_cur[2 * i] - px_ref[2 * i], dy = px_cur[2 * i + 1] - px_ref[2 * i + 1];
    const double e = std::sqrt((dx - sx) * (dx - sx) + (dy - sy) * (dy - sy));
    if (e > worst) worst = e;
    if (error[i] > worst_residual) worst_residual = error[i];
    mx += dx; my += dy; ++n;
  }
  std::printf("%d of %d points tracked: mean shift (%.4f, %.4f) vs (%.4f, %.4f), worst point off by %.4f px, worst residual %.3f grey "
              "levels; median disparity %.4f px vs %.4f\n", (int)n_tracked, N, n ? mx / n : 0.0, n ? my / n : 0.0, sx, sy, worst, worst_residual,
              median, std::sqrt(sx * sx + sy * sy));
  for (void* p : {d_slots, d_px_ref, d_px_cur, d_status, d_error, d_f, d_disp, d_n, d_med, d_store}) svo_hip_free(p);
  svo_hip_stream_destroy(stream);
  if (n != n_tracked || n < N * 9 / 10 || !(worst <= 0.05)) { std::fprintf(stderr, "FAILED\n"); return 1; }
  std::puts("OK");
  return 0;
}
