// TEST INFRASTRUCTURE: rpg_svo_amd/csrc/keyframe_insert.hip compiled for the host (tests/host/hip_emu.h); with
// emu_tu_common.cpp and keyframe_insert_main.cpp a unit of K12's stand-alone programs (tests/keyframe_insert_host.py).
#include "hip_emu.h"
#include "../../rpg_svo_amd/csrc/keyframe_insert.hip"
