// TEST INFRASTRUCTURE: a stand-alone program (its own main) that runs rpg_svo_amd/csrc/keyframe_insert.hip in its
// host-emulated form (emu_tu_keyframe_insert.cpp, emu_tu_common.cpp) on the case files tests/keyframe_insert_host.py writes.
//
//   keyframe_insert_prog run <schedule> <case file> <result file> [<case file> <result file> ...]
//       schedule: inorder | reverse | waves -- the emulator's order of the work-items, set (SVO_EMU_SCHEDULE) before the
//       first launch.  A case file: ten int32 (magic, B, n_stride, K, F, P, R, width, height, calls), the arrays of
//       svo_hip_seq_map in the struct's order, then per call the arrays of svo_hip_keyframe_insert_in.  Every array is
//       copied into a heap block of exactly its size between two guard bands; the outputs start poisoned.  The result file:
//       per call the return code, the state's arrays and the five outputs.
//   keyframe_insert_prog args
//       the argument errors of the entry (SVO_HIP_EINVAL / SVO_HIP_ERANGE, B == 0), none of which may touch a buffer.
// Built by tests/emu_build.py's build_program, with -fsanitize=address,undefined for tests/test_keyframe_insert_sanitized.py.
// Prints "ok" as its last line when every call returned and every guard band is intact.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "svo_hip.h"

namespace {

constexpr size_t GUARD = 512;  // bytes of 0xA5 on either side of every array
constexpr int32_t MAGIC = 0x4b313249;

struct Block {  // an array of exactly `bytes` bytes between two guard bands
  std::unique_ptr<uint8_t[]> raw;
  size_t bytes = 0;
  void init(size_t n, int fill) {
    bytes = n;
    raw.reset(new uint8_t[n + 2 * GUARD]);
    std::memset(raw.get(), 0xA5, n + 2 * GUARD);
    std::memset(raw.get() + GUARD, fill, n);
  }
  uint8_t* data() { return raw.get() + GUARD; }
  bool intact() const {
    for (size_t i = 0; i < GUARD; ++i)
      if (raw[i] != 0xA5 || raw[GUARD + bytes + i] != 0xA5) return false;
    return true;
  }
  bool all(int v) const {
    for (size_t i = 0; i < bytes; ++i)
      if (raw[GUARD + i] != (uint8_t)v) return false;
    return true;
  }
};

struct Dims {
  int32_t B, n_stride, K, F, P, R, width, height, calls;
};

// bytes of the 19 arrays of svo_hip_seq_map, of the 11 inputs and of the 5 outputs, in the structs' order
std::vector<size_t> state_bytes(const Dims& d) {
  const size_t B = d.B, K = d.K, F = d.F, P = d.P, R = d.R, kf = B * K;
  return {4 * B, 4 * kf, 4 * kf, 96 * kf, 4 * kf, 20 * kf, 16 * kf * F, 24 * kf * F, 4 * kf * F, 4 * kf * F,
          24 * B * P, 4 * B * P, 4 * B * P, 4 * B * P, 4 * B * P * R, 4 * B * P * R, 4 * B * P * R, 16 * B * P * R, 24 * B * P * R};
}
std::vector<size_t> input_bytes(const Dims& d) {
  const size_t B = d.B, n = d.n_stride;
  return {4 * B, 4 * B, 16 * B * n, 24 * B * n, 4 * B * n, B * n, 4 * B * n, 96 * B, 4 * B, 20 * B, 4 * B};
}

svo_hip_seq_map map_of(const Dims& d, std::vector<Block>& s) {
  svo_hip_seq_map m;
  m.kf_stride = d.K; m.ftr_stride = d.F; m.pt_stride = d.P; m.obs_stride = d.R;
  auto i32 = [&](int k) { return reinterpret_cast<int32_t*>(s[k].data()); };
  auto f64 = [&](int k) { return reinterpret_cast<double*>(s[k].data()); };
  m.d_n_kf = i32(0); m.d_kf_list = i32(1); m.d_kf_store_slot = i32(2); m.d_kf_T = f64(3); m.d_kf_n_fts = i32(4); m.d_kf_key_pts = i32(5);
  m.d_ftr_px = f64(6); m.d_ftr_f = f64(7); m.d_ftr_level = i32(8); m.d_ftr_point = i32(9);
  m.d_pt_pos = f64(10); m.d_pt_type = i32(11); m.d_pt_order = i32(12); m.d_pt_n_obs = i32(13);
  m.d_obs_kf = i32(14); m.d_obs_row = i32(15); m.d_obs_level = i32(16); m.d_obs_px = f64(17); m.d_obs_f = f64(18);
  return m;
}
svo_hip_keyframe_insert_in in_of(std::vector<Block>& a) {
  auto i32 = [&](int k) { return reinterpret_cast<const int32_t*>(a[k].data()); };
  auto f64 = [&](int k) { return reinterpret_cast<const double*>(a[k].data()); };
  return {i32(0), i32(1), f64(2), f64(3), i32(4), a[5].data(), i32(6), f64(7), i32(8), i32(9), i32(10)};
}
svo_hip_keyframe_insert_out out_of(std::vector<Block>& o) {
  auto i32 = [&](int k) { return reinterpret_cast<int32_t*>(o[k].data()); };
  return {i32(0), i32(1), i32(2), i32(3), i32(4)};
}

svo_hip_camera camera(int width, int height) {
  svo_hip_camera cam{};
  cam.fx = cam.fy = 100.0; cam.cx = 0.5 * width; cam.cy = 0.5 * height; cam.width = width; cam.height = height; cam.model = SVO_HIP_CAM_PINHOLE;
  return cam;
}

int run_file(const char* in_path, const char* out_path) {
  FILE* fi = std::fopen(in_path, "rb");
  if (!fi) return std::printf("cannot open %s\n", in_path), 1;
  int32_t head[10];
  if (std::fread(head, 4, 10, fi) != 10 || head[0] != MAGIC) return std::printf("%s is no case file\n", in_path), 1;
  const Dims d{head[1], head[2], head[3], head[4], head[5], head[6], head[7], head[8], head[9]};
  std::vector<Block> state(19), inputs(11), outputs(5);
  const std::vector<size_t> sb = state_bytes(d), ib = input_bytes(d);
  for (int k = 0; k < 19; ++k) {
    state[k].init(sb[k], 0);
    if (std::fread(state[k].data(), 1, sb[k], fi) != sb[k]) return std::printf("%s is short\n", in_path), 1;
  }
  FILE* fo = std::fopen(out_path, "wb");
  if (!fo) return std::printf("cannot write %s\n", out_path), 1;
  const svo_hip_camera cam = camera(d.width, d.height);
  for (int c = 0; c < d.calls; ++c) {
    for (int k = 0; k < 11; ++k) {
      inputs[k].init(ib[k], 0);
      if (std::fread(inputs[k].data(), 1, ib[k], fi) != ib[k]) return std::printf("%s is short\n", in_path), 1;
    }
    for (int k = 0; k < 5; ++k) outputs[k].init(4 * (size_t)d.B, 0x55);
    const svo_hip_seq_map m = map_of(d, state);
    const svo_hip_keyframe_insert_in in = in_of(inputs);
    const svo_hip_keyframe_insert_out o = out_of(outputs);
    const int32_t rc = svo_hip_keyframe_insert(&cam, d.B, d.n_stride, &m, &in, &o, nullptr);
    for (auto* set : {&state, &inputs, &outputs})
      for (Block& b : *set)
        if (!b.intact()) return std::printf("%s, call %d: a guard band was written\n", in_path, c), 1;
    std::fwrite(&rc, 4, 1, fo);
    for (Block& b : state) std::fwrite(b.data(), 1, b.bytes, fo);
    for (Block& b : outputs) std::fwrite(b.data(), 1, b.bytes, fo);
  }
  std::fclose(fi);
  std::fclose(fo);
  return 0;
}

// the argument errors: none touches a buffer
int run_args() {
  const Dims d{2, 8, 3, 6, 10, 3, 160, 120, 1};
  std::vector<Block> state(19), inputs(11), outputs(5);
  const std::vector<size_t> sb = state_bytes(d), ib = input_bytes(d);
  for (int k = 0; k < 19; ++k) state[k].init(sb[k], 0x55);
  for (int k = 0; k < 11; ++k) inputs[k].init(ib[k], 0);
  for (int k = 0; k < 5; ++k) outputs[k].init(4 * (size_t)d.B, 0x55);
  const svo_hip_camera cam = camera(d.width, d.height);
  const svo_hip_seq_map m = map_of(d, state);
  const svo_hip_keyframe_insert_in in = in_of(inputs);
  const svo_hip_keyframe_insert_out o = out_of(outputs);
  int bad = 0;
  auto expect = [&](const char* what, int got, int want) {
    bool clean = true;
    for (Block& b : state) clean = clean && b.all(0x55) && b.intact();
    for (Block& b : outputs) clean = clean && b.all(0x55) && b.intact();
    if (got != want || !clean) ++bad, std::printf("%s: returned %d, expected %d%s\n", what, got, want, clean ? "" : "; a buffer was written");
  };
  expect("B == 0", svo_hip_keyframe_insert(&cam, 0, d.n_stride, &m, &in, &o, nullptr), SVO_HIP_OK);
  expect("B < 0", svo_hip_keyframe_insert(&cam, -1, d.n_stride, &m, &in, &o, nullptr), SVO_HIP_EINVAL);
  expect("n_stride < 0", svo_hip_keyframe_insert(&cam, d.B, -1, &m, &in, &o, nullptr), SVO_HIP_EINVAL);
  expect("n_stride > 1024", svo_hip_keyframe_insert(&cam, d.B, 1025, &m, &in, &o, nullptr), SVO_HIP_ERANGE);
  expect("no camera", svo_hip_keyframe_insert(nullptr, d.B, d.n_stride, &m, &in, &o, nullptr), SVO_HIP_EINVAL);
  expect("no map", svo_hip_keyframe_insert(&cam, d.B, d.n_stride, nullptr, &in, &o, nullptr), SVO_HIP_EINVAL);
  expect("no inputs", svo_hip_keyframe_insert(&cam, d.B, d.n_stride, &m, nullptr, &o, nullptr), SVO_HIP_EINVAL);
  expect("no outputs", svo_hip_keyframe_insert(&cam, d.B, d.n_stride, &m, &in, nullptr, nullptr), SVO_HIP_EINVAL);
  const int32_t limit[4] = {SVO_HIP_SEQ_MAP_MAX_KFS, SVO_HIP_SEQ_MAP_MAX_FTS, SVO_HIP_SEQ_MAP_MAX_PTS, SVO_HIP_SEQ_MAP_MAX_OBS};
  for (int k = 0; k < 4; ++k) {
    for (int32_t v : {0, -1, limit[k] + 1}) {
      svo_hip_seq_map mm = m;
      (k == 0 ? mm.kf_stride : k == 1 ? mm.ftr_stride : k == 2 ? mm.pt_stride : mm.obs_stride) = v;
      expect("a capacity out of range", svo_hip_keyframe_insert(&cam, d.B, d.n_stride, &mm, &in, &o, nullptr), v > 0 ? SVO_HIP_ERANGE : SVO_HIP_EINVAL);
    }
  }
  expect("B * P * R beyond 2^31", svo_hip_keyframe_insert(&cam, 0x7fffffff, d.n_stride, &m, &in, &o, nullptr), SVO_HIP_ERANGE);
  for (int k = 0; k < 19; ++k) {  // every pointer of the state, of the inputs, of the outputs
    svo_hip_seq_map mm = m;
    void** p = reinterpret_cast<void**>(reinterpret_cast<uint8_t*>(&mm) + 16) + k;
    *p = nullptr;
    expect("a null state pointer", svo_hip_keyframe_insert(&cam, d.B, d.n_stride, &mm, &in, &o, nullptr), SVO_HIP_EINVAL);
  }
  for (int k = 0; k < 11; ++k) {
    svo_hip_keyframe_insert_in ii = in;
    reinterpret_cast<const void**>(&ii)[k] = nullptr;
    expect("a null input pointer", svo_hip_keyframe_insert(&cam, d.B, d.n_stride, &m, &ii, &o, nullptr), SVO_HIP_EINVAL);
  }
  for (int k = 0; k < 5; ++k) {
    svo_hip_keyframe_insert_out oo = o;
    reinterpret_cast<void**>(&oo)[k] = nullptr;
    expect("a null output pointer", svo_hip_keyframe_insert(&cam, d.B, d.n_stride, &m, &in, &oo, nullptr), SVO_HIP_EINVAL);
  }
  std::printf("argument errors: %d wrong\n", bad);
  return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "args") {
    if (run_args()) return 1;
  } else if (mode == "run" && argc >= 5 && (argc - 3) % 2 == 0) {
    const std::string schedule = argv[2];
    if (schedule != "inorder" && schedule != "reverse" && schedule != "waves") return std::printf("unknown schedule %s\n", argv[2]), 2;
    if (schedule == "inorder") unsetenv("SVO_EMU_SCHEDULE");
    else setenv("SVO_EMU_SCHEDULE", argv[2], 1);
    for (int k = 3; k + 1 < argc; k += 2)
      if (run_file(argv[k], argv[k + 1])) return 1;
    std::printf("ran %d case files, schedule %s\n", (argc - 3) / 2, argv[2]);
  } else {
    return std::printf("usage: %s run <inorder|reverse|waves> <case> <result> ... | args\n", argv[0]), 2;
  }
  std::printf("ok\n");
  return 0;
}
