"""K10's memory accesses and arithmetic under AddressSanitizer and UndefinedBehaviorSanitizer, without a GPU and without
loading anything into Python: tests/host/first_map_asan_main.cpp is a program of its own that runs the host-emulated
svo_hip_first_map (257 corners, a failed sequence, pixels that are NaN, negative and beyond the grid) and
svo_hip_initialize_seeds (1040 cells) on heap buffers of exactly the documented sizes.  tests/emu_build.py
compiles it with -fsanitize=address,undefined; it must exit 0 with no report."""
import subprocess

from emu_build import build_first_map_asan_program


def test_first_map_and_seeds_stay_inside_their_buffers():
    exe = build_first_map_asan_program()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env={"ASAN_OPTIONS": "detect_leaks=0"})
    print(r.stdout)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout, r.stderr[-2000:])
