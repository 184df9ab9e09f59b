// TEST INFRASTRUCTURE: a stand-alone program (its own main) that pushes the table of tests/pose_lds_cases.py through the
// host-emulated pose optimizer (pose_lds_asan_tu_wave.cpp: the wave kernel, pose_lds_asan_tu_ordered.cpp: the C ABI entries and
// the ordered kernel; emu_tu_common.cpp) on heap buffers of exactly the sizes the C ABI asks for and dynamic LDS of exactly the
// byte count of each launch (pose_lds_asan_lds.h).  Built with -fsanitize=address,undefined by tests/pose_lds_cases.py: a
// load or store outside a buffer or the LDS block, or undefined behaviour in the kernels, stops it with a report and a non-zero
// exit status.
// usage: pose_lds_asan IN OUT
//   IN:  per row  int32 ns, B, n_iter; double thresh; svo_hip_camera; int32 n[B]; double f[B][ns][3]; int32 level[B][ns];
//        double pos[B][ns][3]; uint8 has_point[B][ns]; double T[B][12]          (rows follow each other to the end of the file)
//   OUT: per row and call (svo_hip_pose_optimize with n_iter, svo_hip_pose_optimize_deferred with n_iter = 0)
//        double T[B][12]; double Cov[B][36]; double stats[B][4]; int32 ran[B]; uint8 has_point[B][ns]
// Exits 0, the last line "ok", when every call returned SVO_HIP_OK.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "svo_hip.h"

namespace {

template <typename T>
bool rd(std::FILE* f, std::vector<T>& v) { return std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T>
bool wr(std::FILE* f, const std::vector<T>& v) { return std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return std::printf("usage: %s IN OUT\n", argv[0]), 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return std::printf("cannot open %s / %s\n", argv[1], argv[2]), 2;
  int rows = 0;
  for (;;) {
    int32_t head[3];
    if (std::fread(head, sizeof(int32_t), 3, in) != 3) break;
    const int ns = head[0], B = head[1], n_iter = head[2];
    double thresh;
    svo_hip_camera cam;
    if (ns < 1 || B < 1 || std::fread(&thresh, sizeof(double), 1, in) != 1 || std::fread(&cam, sizeof(cam), 1, in) != 1)
      return std::printf("row %d: bad header\n", rows), 2;
    std::vector<int32_t> n(B), level((size_t)B * ns);
    std::vector<double> f((size_t)B * ns * 3), pos((size_t)B * ns * 3), T0((size_t)B * 12);
    std::vector<uint8_t> hp0((size_t)B * ns);
    if (!rd(in, n) || !rd(in, f) || !rd(in, level) || !rd(in, pos) || !rd(in, hp0) || !rd(in, T0)) return std::printf("row %d: short file\n", rows), 2;
    for (int leg = 0; leg < 2; ++leg) {
      // results on heap blocks of their own, exactly as long as the C ABI says
      std::vector<double> T(T0), Cov((size_t)B * 36, 0.0), stats((size_t)B * 4, 0.0);
      std::vector<int32_t> ran(B, -1);
      std::vector<uint8_t> hp(hp0);
      const int it = leg == 0 ? n_iter : 0;
      const int rc = (leg & 1 ? svo_hip_pose_optimize_deferred : svo_hip_pose_optimize)(
          &cam, B, n.data(), ns, f.data(), level.data(), pos.data(), hp.data(), thresh, it, T.data(), Cov.data(), stats.data(), ran.data(), nullptr);
      if (rc != SVO_HIP_OK) return std::printf("row of %d, leg %d: returned %d\n", ns, leg, rc), 1;
      if (!wr(out, T) || !wr(out, Cov) || !wr(out, stats) || !wr(out, ran) || !wr(out, hp)) return std::printf("cannot write\n"), 2;
    }
    std::printf("row of %d observations: %d frames, two calls\n", ns, B);
    ++rows;
  }
  std::fclose(in);
  if (std::fclose(out) != 0 || rows == 0) return std::printf("no row / write failed\n"), 2;
  std::printf("ok\n");
  return 0;
}
