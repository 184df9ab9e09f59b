// TEST INFRASTRUCTURE: the dynamic LDS of the stand-alone sanitizer program of the pose optimizer (pose_lds_asan_main.cpp).
// hip_emu.h serves every launch's dynamic LDS from one buffer with room for a whole CU, where an access beyond the launch's
// byte count stays inside the allocation and no sanitizer sees it.  Here every launch gets a heap block of EXACTLY the byte
// count it asked for: AddressSanitizer's red zones stand right behind the last byte the kernel may touch.
#pragma once
#include <cstddef>
#include <memory>

#include "hip_emu.h"

namespace pose_lds_asan {
inline std::unique_ptr<unsigned char[]> g_lds;
inline void fresh(size_t bytes) {
  g_lds.reset();
  g_lds.reset(new unsigned char[bytes ? bytes : 1]);  // (operator new: aligned for a double, which is all the kernels ask)
}
}  // namespace pose_lds_asan

#undef SVO_DYNAMIC_LDS
#undef hipLaunchKernelGGL
#define SVO_DYNAMIC_LDS(type, name) type* const name = reinterpret_cast<type*>(pose_lds_asan::g_lds.get())
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) \
  (pose_lds_asan::fresh((size_t)(shmem)), svo_emu::launch((grid), (block), [&] { kernel(__VA_ARGS__); }))
