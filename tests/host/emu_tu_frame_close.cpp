// TEST INFRASTRUCTURE: rpg_svo_amd/csrc/frame_close.hip compiled for the host (tests/host/hip_emu.h); a unit of the emulated
// library, and with emu_tu_common.cpp of K11's stand-alone sanitizer program (tests/emu_build.py builds both).
#include "hip_emu.h"
#include "../../rpg_svo_amd/csrc/frame_close.hip"
