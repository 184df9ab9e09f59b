// TEST INFRASTRUCTURE: rpg_svo_amd/csrc/first_map.hip compiled for the host (tests/host/hip_emu.h); tests/emu_build_first_map.py
// links it with emu_tu_common.cpp into a library of its own.
#include "hip_emu.h"
#include "../../rpg_svo_amd/csrc/first_map.hip"
