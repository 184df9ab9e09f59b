"""K11's memory accesses and arithmetic under AddressSanitizer and UndefinedBehaviorSanitizer, without a GPU and without
loading anything into Python: tests/host/frame_close_asan_main.cpp is a program of its own that runs the host-emulated
svo_hip_frame_close on heap buffers of exactly the documented sizes: 257 and 1024 rows with 64 keyframes, row counts below,
at and beyond the stride, rows without a point, pixels that are NaN, negative and beyond the grid.
tests/emu_build_frame_close.py compiles it with -fsanitize=address,undefined; it must exit 0 with no report."""
import subprocess

from emu_build_frame_close import build_frame_close_asan_program


def test_frame_close_stays_inside_its_buffers():
    exe = build_frame_close_asan_program()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env={"ASAN_OPTIONS": "detect_leaks=0"})
    print(r.stdout)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout, r.stderr[-2000:])
