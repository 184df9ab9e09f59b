// TEST INFRASTRUCTURE: a stand-alone program (its own main) that runs svo_hip_reproject_map in its host-emulated form
// (emu_tu_map_mirror.cpp, emu_tu_common.cpp) on the steps tests/map_mirror_cases.py writes (write_steps: the limit cases -- a cell of
// more than 600 entries, 4096 / 4097 points inside the frame out of up to 8192 entries, 2048 cells, the key ranges at their
// ends), every map, patch and output array a heap buffer of exactly its size.  Built with -fsanitize=address,undefined by
// tests/emu_build.py: a load or store outside a buffer (the oracle comparison cannot see a read one past the end that happens to
// be harmless) or undefined behaviour in the kernel stops it with a report and a non-zero exit status.  The outputs start poisoned
// (ints 0x55555555, doubles NaN) and are written back for the rule of tests/map_mirror_cases.py (read_outputs, check_step).
//   map_mirror_asan <steps file> <outputs file>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "svo_hip.h"

namespace {

template <class T>
bool read(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

template <class T>
bool write(std::FILE* f, const std::vector<T>& v) {
  return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int run_step(std::FILE* in, std::FILE* out, int step) {
  std::vector<int32_t> h;
  std::vector<double> k;
  if (!read(in, h, 14) || !read(in, k, 9)) return std::printf("step %d: short header\n", step), 1;
  const int n_frames = h[3], cur = h[4], P = h[5], O = h[6], cell_size = h[7], n_cols = h[8], n_rows = h[9], first_cell = h[10],
            max_cells = h[11], max_visits = h[12], max_trials = h[13], n_cells = n_cols * n_rows;
  svo_hip_camera cam{};
  cam.model = h[0]; cam.width = h[1]; cam.height = h[2];
  cam.fx = k[0]; cam.fy = k[1]; cam.cx = k[2]; cam.cy = k[3];
  for (int i = 0; i < 5; ++i) cam.d[i] = k[4 + i];
  std::vector<double> T, pos, obs_px, obs_f, obs_grad;
  std::vector<int32_t> kf_rank, type, order, obs_begin, obs_count, obs_frame, obs_order, obs_level, obs_type32, cell_rank;
  if (!read(in, T, (size_t)n_frames * 12) || !read(in, kf_rank, n_frames) || !read(in, pos, (size_t)P * 3) || !read(in, type, P) ||
      !read(in, order, P) || !read(in, obs_begin, P) || !read(in, obs_count, P) || !read(in, obs_frame, O) || !read(in, obs_order, O) ||
      !read(in, obs_level, O) || !read(in, obs_type32, O) || !read(in, obs_px, (size_t)O * 2) || !read(in, obs_f, (size_t)O * 3) ||
      !read(in, obs_grad, (size_t)O * 2) || !read(in, cell_rank, n_cells))
    return std::printf("step %d: short arrays\n", step), 1;
  std::vector<uint8_t> obs_type(obs_type32.begin(), obs_type32.end());
  // the mirror, empty: the whole map arrives as the call's patch
  std::vector<double> m_pos((size_t)P * 3), m_px((size_t)O * 2), m_f((size_t)O * 3), m_grad((size_t)O * 2);
  std::vector<int32_t> m_type(P), m_order(P), m_begin(P), m_count(P), m_frame(O), m_word(O), m_level(O), p_index(P), o_index(O);
  std::vector<uint8_t> m_otype(O);
  for (int i = 0; i < P; ++i) p_index[i] = i;
  for (int i = 0; i < O; ++i) o_index[i] = i;
  svo_hip_map map{P, O, m_pos.data(), m_type.data(), m_order.data(), m_begin.data(), m_count.data(), m_frame.data(), m_word.data(),
                  m_level.data(), m_otype.data(), m_px.data(), m_f.data(), m_grad.data()};
  svo_hip_map_patch patch{};
  patch.n_points = P; patch.n_obs = O;
  patch.d_index = p_index.data(); patch.d_pos = pos.data(); patch.d_type = type.data(); patch.d_order = order.data();
  patch.d_obs_begin = obs_begin.data(); patch.d_obs_count = obs_count.data(); patch.d_obs_index = o_index.data(); patch.d_obs_order = obs_order.data();
  patch.obs.d_frame = obs_frame.data(); patch.obs.d_level = obs_level.data(); patch.obs.d_type = obs_type.data(); patch.obs.d_px = obs_px.data();
  patch.obs.d_f = obs_f.data(); patch.obs.d_grad = obs_grad.data();
  svo_hip_frames frames{};
  frames.n_frames = n_frames; frames.d_T_f_w = T.data();
  svo_hip_grid grid{cell_size, n_cols, n_rows, n_cells, cell_rank.data()};
  const int32_t poison = 0x55555555;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<int32_t> header(SVO_HIP_REPROJ_HEADER, poison), point_cell(P, poison), kf_count(n_frames, poison), visit_point(max_visits, poison),
      visit_cell(max_visits, poison), visit_trial(max_visits, poison), trial_cur(max_trials, poison), trial_begin(max_trials, poison),
      trial_end(max_trials, poison), trial_cell(max_trials, poison);
  std::vector<double> point_px((size_t)P * 2, nan), trial_pos((size_t)max_trials * 3, nan), trial_px((size_t)max_trials * 2, nan);
  svo_hip_reprojection o{header.data(), point_cell.data(), point_px.data(), kf_count.data(), visit_point.data(), visit_cell.data(),
                         visit_trial.data(), trial_cur.data(), trial_pos.data(), trial_begin.data(), trial_end.data(), trial_cell.data(),
                         trial_px.data()};
  const int32_t rc = svo_hip_reproject_map(&cam, &frames, cur, kf_rank.data(), &map, &patch, &grid, first_cell, max_cells, max_visits,
                                           max_trials, &o, nullptr);
  std::printf("step %d: %d entries, %d cells, rc %d, status %d, %d in the frame, %d visits, %d trials\n", step, P, n_cells, rc, header[0],
              header[1], header[2], header[3]);
  if (std::fwrite(&rc, sizeof rc, 1, out) != 1) return 1;
  const bool ok = write(out, header) && write(out, point_cell) && write(out, point_px) && write(out, kf_count) && write(out, visit_point) &&
                  write(out, visit_cell) && write(out, visit_trial) && write(out, trial_cur) && write(out, trial_pos) && write(out, trial_begin) &&
                  write(out, trial_end) && write(out, trial_cell) && write(out, trial_px);
  return ok && rc == SVO_HIP_OK ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return std::printf("usage: map_mirror_asan <steps file> <outputs file>\n"), 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return std::printf("cannot open the files\n"), 2;
  int32_t n = 0;
  if (std::fread(&n, sizeof n, 1, in) != 1) return 2;
  for (int s = 0; s < n; ++s)
    if (run_step(in, out, s)) return 1;
  std::fclose(in);
  std::fclose(out);
  std::printf("ok\n");
  return 0;
}
