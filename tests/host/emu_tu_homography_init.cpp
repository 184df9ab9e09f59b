// TEST INFRASTRUCTURE: rpg_svo_amd/csrc/homography_init.hip compiled for the host (tests/host/hip_emu.h);
// tests/homography_emu_build.py links it with the common unit of the emulated build.
#include "hip_emu.h"
#include "../../rpg_svo_amd/csrc/homography_init.hip"
