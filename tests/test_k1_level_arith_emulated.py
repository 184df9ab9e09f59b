"""The per-level arithmetic of K1 -- the factored patch Hessian (csrc/sia_common.h: sia_patch_hessian, its three S values masked
by membership) and the packed template of a level (sia_ref_tile_packed) -- through the host-emulated library in both widths of
K1 (tests/k1_emulated.py), on the frames tests/k1_cases.py builds for it, against the oracle under that module's rule and its
emulated profiles: poses to 1e-5 in SE(3) log-norm, tracked counts identical, H to 1e-4 of its largest entry.
(The emulation has no frame split over several workgroups: the 600-patch frame runs on the 1024-lane workgroup here and
through the split kernel in tests/test_k1_level_arith_gpu.py.)"""
import pytest

import k1_cases as k1
import k1_emulated


@pytest.fixture(scope="module", params=k1_emulated.K1_BUILDS, ids=k1_emulated.K1_BUILD_IDS)
def emu(request):
    return k1_emulated.Emulated(request.param)


@pytest.fixture(scope="module")
def emu_default():
    return k1_emulated.Emulated(0)


@pytest.mark.parametrize("name", k1.LEVEL_ARITH_FRAMES)
def test_emulated_frames_for_the_level_arithmetic(emu, oracle, name):
    c = k1.case(name)
    k1.verify_pair(oracle, emu.name, name, c.schedules[0], emu.run(c, c.schedules[0]))


@pytest.mark.parametrize("n_patches", [60, 190])
def test_emulated_wave_kernel_patch_hessian(emu_default, oracle, n_patches):
    """sparse_align_wave.hip calls the helper with T = float, once per patch of a lane (one and three patches per lane)"""
    c = k1.case(f"wave_arith_{n_patches}")
    k1.verify_pair(oracle, k1.EMU_WAVE, c.name, c.schedules[0], emu_default.run(c, c.schedules[0], kernel="wave"))
