// TEST INFRASTRUCTURE: a stand-alone program (its own main) that runs both entries of rpg_svo_amd/csrc/first_map.hip in their
// host-emulated form (emu_tu_first_map.cpp, emu_tu_common.cpp) on heap buffers of exactly the sizes the C ABI asks for: 257
// corners in three sequences (two chunks of the compaction loop, a failed sequence in the middle, pixels that are NaN,
// negative and beyond the grid) and 1040 cells in two keyframes (five blocks of the running offset).  Built with
// -fsanitize=address,undefined by tests/emu_build.py: a load or store outside a buffer, or undefined behaviour in
// the kernels, stops it with a report and a non-zero exit status.  Exits 0 when both calls return SVO_HIP_OK with the counts
// the inputs were made for.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "svo_hip.h"

namespace {

uint32_t g_state = 12345u;
double uniform() {  // xorshift32 in [0, 1)
  g_state ^= g_state << 13;
  g_state ^= g_state >> 17;
  g_state ^= g_state << 5;
  return (double)g_state / 4294967296.0;
}

int run_first_map() {
  const int n_seq = 3, n_pts = 257, cell_size = 30, cols = 6, rows = 4, cells = cols * rows;
  svo_hip_camera cam{};
  cam.fx = cam.fy = 140.0; cam.cx = 79.5; cam.cy = 59.5; cam.width = 160; cam.height = 120; cam.model = SVO_HIP_CAM_PINHOLE;
  std::vector<int32_t> result = {SVO_HIP_INIT_SUCCESS, SVO_HIP_INIT_NO_KEYFRAME, SVO_HIP_INIT_SUCCESS};
  std::vector<uint8_t> ok((size_t)n_seq * n_pts);
  std::vector<double> point_w((size_t)n_seq * n_pts * 3), f_ref(point_w.size()), f_cur(point_w.size());
  std::vector<float> px_ref((size_t)n_seq * n_pts * 2), px_cur(px_ref.size());
  std::vector<double> T_ref((size_t)n_seq * 12, 0.0), T_cur((size_t)n_seq * 12, 0.0);
  int expect[3] = {0, 0, 0};
  for (int s = 0; s < n_seq; ++s) {
    for (int k = 0; k < 3; ++k) T_ref[12 * s + 4 * k] = T_cur[12 * s + 4 * k] = 1.0;
    T_cur[12 * s + 9] = 0.25;
    for (int i = 0; i < n_pts; ++i) {
      const size_t g = (size_t)s * n_pts + i;
      ok[g] = uniform() < 0.7 ? 1 : 0;
      if (ok[g] && result[s] == SVO_HIP_INIT_SUCCESS) ++expect[s];
      for (int e = 0; e < 3; ++e) {
        point_w[3 * g + e] = uniform() * 2.0 + (e == 2 ? 1.0 : -1.0);
        f_ref[3 * g + e] = f_cur[3 * g + e] = e == 2 ? 1.0 : uniform() - 0.5;
      }
      px_ref[2 * g] = (float)(uniform() * 159.0); px_ref[2 * g + 1] = (float)(uniform() * 119.0);
      px_cur[2 * g] = (float)(uniform() * 159.0); px_cur[2 * g + 1] = (float)(uniform() * 119.0);
    }
    const float bad[6][2] = {{NAN, 5.f}, {5.f, -INFINITY}, {-95.f, 5.f}, {5.f, 4000.f}, {3e9f, 3e9f}, {-3e9f, 1.f}};
    for (int k = 0; k < 6; ++k) {
      const size_t g = (size_t)s * n_pts + 40 * k + 3;
      px_cur[2 * g] = bad[k][0]; px_cur[2 * g + 1] = bad[k][1];
      px_ref[2 * g] = bad[k][1]; px_ref[2 * g + 1] = bad[k][0];
    }
  }
  std::vector<int32_t> n_points(n_seq), src_index((size_t)n_seq * n_pts), key_pts((size_t)n_seq * 10);
  std::vector<double> pos((size_t)n_seq * n_pts * 3), px((size_t)n_seq * 2 * n_pts * 2), f((size_t)n_seq * 2 * n_pts * 3);
  std::vector<double> depth_mean(n_seq), depth_min(n_seq), xyz_ref((size_t)n_seq * n_pts * 3);
  std::vector<uint8_t> occupancy((size_t)n_seq * cells);
  svo_hip_first_map_out o{n_points.data(), src_index.data(), pos.data(), px.data(), f.data(), key_pts.data(), depth_mean.data(),
                          depth_min.data(), xyz_ref.data(), occupancy.data()};
  const int rc = svo_hip_first_map(&cam, n_seq, n_pts, result.data(), ok.data(), point_w.data(), px_ref.data(), px_cur.data(), f_ref.data(),
                                   f_cur.data(), T_ref.data(), T_cur.data(), cell_size, cols, rows, cells, &o, nullptr);
  if (rc != SVO_HIP_OK) return std::printf("svo_hip_first_map returned %d\n", rc), 1;
  for (int s = 0; s < n_seq; ++s)
    if (n_points[s] != expect[s]) return std::printf("sequence %d: %d points, expected %d\n", s, n_points[s], expect[s]), 1;
  std::printf("first map: %d / %d / %d points, depth %.3f / %.3f\n", n_points[0], n_points[1], n_points[2], depth_mean[0], depth_min[0]);
  return 0;
}

int run_seeds() {
  const int n_frames = 2, n_cells = 1040, stride = 1040;
  svo_hip_camera cam{};
  cam.fx = cam.fy = 315.5; cam.cx = 376.0; cam.cy = 240.0; cam.width = 752; cam.height = 480; cam.model = SVO_HIP_CAM_PINHOLE;
  std::vector<int32_t> xy((size_t)n_frames * n_cells * 2), level((size_t)n_frames * n_cells), frame_index = {4, 9};
  std::vector<float> score((size_t)n_frames * n_cells);
  std::vector<double> depth_mean = {1.5, 0.0}, depth_min = {0.4, 0.0};
  int expect[2] = {0, 0};
  for (int fr = 0; fr < n_frames; ++fr)
    for (int c = 0; c < n_cells; ++c) {
      const size_t g = (size_t)fr * n_cells + c;
      const bool has = uniform() < 0.6;
      xy[2 * g] = has ? (int)(uniform() * 752) : -1; xy[2 * g + 1] = has ? (int)(uniform() * 480) : -1;
      level[g] = has ? (int)(uniform() * 3) : 0;
      score[g] = has ? 20.f + (float)(uniform() * 100.0) : 20.f;
      if ((double)score[g] > 20.0) ++expect[fr];
    }
  const size_t n = (size_t)n_frames * stride;
  std::vector<int32_t> n_seeds(n_frames), frame(n), lvl(n), batch_id(n);
  std::vector<uint8_t> type(n);
  std::vector<double> px(2 * n), f(3 * n), grad(2 * n);
  std::vector<float> a(n), b(n), mu(n), z_range(n), sigma2(n);
  svo_hip_seed_init_out o{n_seeds.data(), frame.data(), lvl.data(), type.data(), px.data(), f.data(), grad.data(), a.data(), b.data(),
                          mu.data(), z_range.data(), sigma2.data(), batch_id.data()};
  const int rc = svo_hip_initialize_seeds(&cam, n_frames, n_cells, xy.data(), level.data(), score.data(), 20.0, frame_index.data(),
                                          depth_mean.data(), depth_min.data(), 1, stride, &o, nullptr);
  if (rc != SVO_HIP_OK) return std::printf("svo_hip_initialize_seeds returned %d\n", rc), 1;
  for (int fr = 0; fr < n_frames; ++fr)
    if (n_seeds[fr] != expect[fr]) return std::printf("keyframe %d: %d seeds, expected %d\n", fr, n_seeds[fr], expect[fr]), 1;
  std::printf("seeds: %d / %d, mu %.6f, sigma2 %.6f\n", n_seeds[0], n_seeds[1], mu[0], sigma2[0]);
  return 0;
}

}  // namespace

int main() {
  if (run_first_map() || run_seeds()) return 1;
  std::printf("ok\n");
  return 0;
}
