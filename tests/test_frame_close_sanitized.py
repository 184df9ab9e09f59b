"""K11's memory accesses and arithmetic under AddressSanitizer and UndefinedBehaviorSanitizer, without a GPU and without
loading anything into Python: tests/host/frame_close_asan_main.cpp is a program of its own that runs the host-emulated
svo_hip_frame_close on heap buffers of exactly the documented sizes: 257 and 1024 rows with 64 keyframes, row counts below,
at and beyond the stride, rows without a point, pixels that are NaN, negative and beyond the grid.
tests/emu_build.py compiles it with -fsanitize=address,undefined; it must exit 0 with no report."""
from emu_build import build_program, run_program


def test_frame_close_stays_inside_its_buffers():
    run_program(build_program("frame_close_asan", ("emu_tu_common.cpp", "emu_tu_frame_close.cpp", "frame_close_asan_main.cpp")))
