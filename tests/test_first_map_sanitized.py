"""K10's memory accesses and arithmetic under AddressSanitizer and UndefinedBehaviorSanitizer, without a GPU and without
loading anything into Python: tests/host/first_map_asan_main.cpp is a program of its own that runs the host-emulated
svo_hip_first_map (257 corners, a failed sequence, pixels that are NaN, negative and beyond the grid) and
svo_hip_initialize_seeds (1040 cells) on heap buffers of exactly the documented sizes.  tests/emu_build.py
compiles it with -fsanitize=address,undefined; it must exit 0 with no report."""
from emu_build import build_program, run_program


def test_first_map_and_seeds_stay_inside_their_buffers():
    run_program(build_program("first_map_asan", ("emu_tu_common.cpp", "emu_tu_first_map.cpp", "first_map_asan_main.cpp")))
