"""The per-level arithmetic of K1 (csrc/sia_common.h: sia_patch_hessian, sia_ref_tile_packed, the shared helpers) on the host, without a GPU and
without loading anything into Python: tests/host/k1_level_arith_main.cpp is a program of its own that checks
  (a) the factored patch Hessian [a b] S [a b]' in f64 and f32 against the written-out triple product in long double
      (10 000 random patches, S = 0, a patch on the optical axis; 16 ulp of the sum of the absolute terms), and
  (b) the packed template of a level against the scalar formulas it replaces, bit for bit (10 000 random 7 x 7 windows, sub-pixel
      positions 0 and 1 - 2^-22, constant windows, checkerboards of 0 / 255), and
  (c) the shared helpers of the K1 kernels -- the tile stores and load, sia_jac_rows, sia_jres_partials, sia_weights,
      sia_project<false> against the pinhole formula and sia_project<true> (radtan, atan) against the block sia_kernel keeps
      written out -- against the formulas the kernels held written out before, bit for bit.
Built with the emulated library's compile flags, once plain and once with -fsanitize=address,undefined; it must exit 0, its
last line "ok", with no report."""
import pytest

from emu_build import build_program, run_program


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "address_undefined"])
def test_patch_hessian_and_packed_template(sanitized):
    run_program(build_program("k1_level_arith" + ("_asan" if sanitized else ""), ("k1_level_arith_main.cpp",), sanitize=sanitized,
                              extra_checks=("float-cast-overflow",), deps=(__file__,)))
