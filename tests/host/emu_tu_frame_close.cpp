// TEST INFRASTRUCTURE: rpg_svo_amd/csrc/frame_close.hip compiled for the host (tests/host/hip_emu.h); with emu_tu_common.cpp
// the emulated library of K11 and its stand-alone sanitizer program (tests/emu_build_frame_close.py builds both).
#include "hip_emu.h"
#include "../../rpg_svo_amd/csrc/frame_close.hip"
