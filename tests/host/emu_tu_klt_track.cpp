// TEST INFRASTRUCTURE: rpg_svo_amd/csrc/klt_track.hip compiled for the host (tests/host/hip_emu.h); tests/klt_emu_build.py links it
// with the common, pyramid and matcher units of the emulated build.
#include "hip_emu.h"
#include "../../rpg_svo_amd/csrc/klt_track.hip"
