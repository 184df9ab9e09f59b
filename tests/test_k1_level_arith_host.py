"""The per-level arithmetic of K1 (csrc/sia_common.h: sia_patch_hessian, sia_ref_tile_packed) on the host, without a GPU and
without loading anything into Python: tests/host/k1_level_arith_main.cpp is a program of its own that checks
  (a) the factored patch Hessian [a b] S [a b]' in f64 and f32 against the written-out triple product in long double
      (10 000 random patches, S = 0, a patch on the optical axis; 16 ulp of the sum of the absolute terms), and
  (b) the packed template of a level against the scalar formulas it replaces, bit for bit (10 000 random 7 x 7 windows, sub-pixel
      positions 0 and 1 - 2^-22, constant windows, checkerboards of 0 / 255).
Built with the emulated library's compile flags, once plain and once with -fsanitize=address,undefined; it must exit 0, its
last line "ok", with no report."""
import os
import subprocess

import pytest

import emu_build

ROOT = emu_build.ROOT


def _build(sanitized):
    from rpg_svo_amd.build import DEFAULT_DEFINES
    cxx = emu_build._cxx()
    if not os.path.exists(cxx):
        pytest.skip("no ROCm clang++ to compile the kernels' headers for the host")
    exe = os.path.join(ROOT, "build", "emu", "k1_level_arith" + ("_asan" if sanitized else ""))
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(ROOT, "tests", "host", "k1_level_arith_main.cpp")
    deps = [src, os.path.abspath(__file__), *emu_build._kernel_deps()]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        san = ["-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=undefined",
               "-fno-sanitize=vptr,function", "-fno-omit-frame-pointer", "-g"] if sanitized else []
        subprocess.run([cxx, *emu_build._kernel_cxxflags(DEFAULT_DEFINES), *san, src, "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "address_undefined"])
def test_patch_hessian_and_packed_template(sanitized):
    exe = _build(sanitized)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env={"ASAN_OPTIONS": "detect_leaks=0"})
    print(r.stdout)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-4000:], r.stderr[-2000:])
