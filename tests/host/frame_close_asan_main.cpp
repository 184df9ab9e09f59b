// TEST INFRASTRUCTURE: a stand-alone program (its own main) that runs rpg_svo_amd/csrc/frame_close.hip in its host-emulated
// form (emu_tu_frame_close.cpp, emu_tu_common.cpp) on heap buffers of exactly the sizes the C ABI asks for: 257 and 1024 rows
// per sequence with 64 keyframes, four sequences each whose row counts lie below, at and beyond the stride (and below zero),
// rows without a point, pixels that are NaN, negative and beyond the grid, keyframe counts of 0, 10, 64 and beyond the stride.
// Built with -fsanitize=address,undefined by tests/emu_build.py: a load or store outside a buffer, or undefined
// behaviour in the kernel, stops it with a report and a non-zero exit status.  Exits 0 when both calls return SVO_HIP_OK with
// the point counts the inputs were made for.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "svo_hip.h"

namespace {

uint32_t g_state = 2463534242u;
double uniform() {  // xorshift32 in [0, 1)
  g_state ^= g_state << 13;
  g_state ^= g_state >> 17;
  g_state ^= g_state << 5;
  return (double)g_state / 4294967296.0;
}

int run(int n_stride) {
  const int B = 4, kf_stride = 64, cell_size = 30, cols = 6, rows = 4, cells = cols * rows;
  svo_hip_camera cam{};
  cam.fx = cam.fy = 140.0; cam.cx = 79.5; cam.cy = 59.5; cam.width = 160; cam.height = 120; cam.model = SVO_HIP_CAM_PINHOLE;
  const std::vector<int32_t> n = {n_stride, n_stride + 50, n_stride / 2, -3}, n_kf = {64, 70, 10, 0};
  const std::vector<int32_t> num_obs = {100, 10, 60, 60}, num_obs_last = {110, 60, 200, 60};
  const size_t R = (size_t)B * n_stride;
  std::vector<double> px(2 * R), f(3 * R), pos(3 * R), T((size_t)B * 12, 0.0), T_last((size_t)B * 12, 0.0), kf_T((size_t)B * kf_stride * 12, 0.0);
  std::vector<uint8_t> has_point(R);
  std::vector<int32_t> kf_overlap((size_t)B * kf_stride);
  int expect[4] = {0, 0, 0, 0};
  for (int b = 0; b < B; ++b) {
    for (int k = 0; k < 3; ++k) T[12 * b + 4 * k] = T_last[12 * b + 4 * k] = 1.0;
    T[12 * b + 9] = 0.25;
    const int live = n[b] < 0 ? 0 : (n[b] > n_stride ? n_stride : n[b]);
    for (int j = 0; j < n_stride; ++j) {
      const size_t g = (size_t)b * n_stride + j;
      has_point[g] = uniform() < 0.7 ? 1 : 0;
      if (has_point[g] && j < live) ++expect[b];
      px[2 * g] = uniform() * 159.0; px[2 * g + 1] = uniform() * 119.0;
      for (int e = 0; e < 3; ++e) {
        pos[3 * g + e] = has_point[g] ? uniform() * 2.0 + (e == 2 ? 1.0 : -1.0) : NAN;
        f[3 * g + e] = e == 2 ? 1.0 : uniform() - 0.5;
      }
    }
    const double bad[6][2] = {{NAN, 5.}, {5., -INFINITY}, {-95., 5.}, {5., 4000.}, {3e9, 3e9}, {-3e9, 1.}};
    for (int k = 0; k < 6; ++k) {
      const size_t g = (size_t)b * n_stride + 40 * k + 3;
      px[2 * g] = bad[k][0]; px[2 * g + 1] = bad[k][1];
    }
    for (int i = 0; i < kf_stride; ++i) {
      double* K = &kf_T[((size_t)b * kf_stride + i) * 12];
      for (int k = 0; k < 3; ++k) K[4 * k] = 1.0;
      K[9] = uniform() - 0.5; K[10] = uniform() - 0.5; K[11] = uniform() - 0.5;
      kf_overlap[(size_t)b * kf_stride + i] = (i % 3) ? i : -1;
    }
  }
  std::vector<int32_t> gate(B), quality(B), result(B), nobs_out(B), kf_block(B), key_pts((size_t)B * 5), kf_remove(B);
  std::vector<double> T_out((size_t)B * 12), depth_mean(B), depth_min(B), xyz_ref(3 * R);
  std::vector<uint8_t> valid(R), occupancy((size_t)B * cells);
  svo_hip_frame_close_params p;
  if (svo_hip_frame_close_params_default(&p) != SVO_HIP_OK) return std::printf("no default parameters\n"), 1;
  const svo_hip_frame_close_in in{n.data(), px.data(), f.data(), pos.data(), has_point.data(), T.data(), T_last.data(), num_obs.data(),
                                  num_obs_last.data(), n_kf.data(), kf_T.data(), kf_overlap.data()};
  const svo_hip_frame_close_out o{gate.data(), quality.data(), result.data(), T_out.data(), nobs_out.data(), depth_mean.data(), depth_min.data(),
                                  kf_block.data(), valid.data(), xyz_ref.data(), key_pts.data(), occupancy.data(), kf_remove.data()};
  const int rc = svo_hip_frame_close(&cam, B, n_stride, kf_stride, &in, cell_size, cols, rows, cells, &p, &o, nullptr);
  if (rc != SVO_HIP_OK) return std::printf("svo_hip_frame_close returned %d\n", rc), 1;
  for (int b = 0; b < B; ++b)
    if (nobs_out[b] != expect[b]) return std::printf("sequence %d: %d points, expected %d\n", b, nobs_out[b], expect[b]), 1;
  if (gate[0] != 0 || gate[1] != 2 || gate[2] != 3 || gate[3] != 1) return std::printf("gates %d %d %d %d\n", gate[0], gate[1], gate[2], gate[3]), 1;
  std::printf("frame close, %d rows: %d / %d / %d / %d points, depth %.3f / %.3f, block %d, remove %d\n", n_stride, nobs_out[0], nobs_out[1],
              nobs_out[2], nobs_out[3], depth_mean[0], depth_min[0], kf_block[0], kf_remove[0]);
  return 0;
}

}  // namespace

int main() {
  if (run(257) || run(1024)) return 1;
  std::printf("ok\n");
  return 0;
}
