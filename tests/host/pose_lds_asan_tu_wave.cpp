// TEST INFRASTRUCTURE: rpg_svo_amd/csrc/pose_optimizer_wave.hip compiled for the host with exactly sized dynamic LDS
// (pose_lds_asan_lds.h); a unit of the stand-alone sanitizer program of the pose optimizer.
#include "pose_lds_asan_lds.h"
#include "../../rpg_svo_amd/csrc/pose_optimizer_wave.hip"
