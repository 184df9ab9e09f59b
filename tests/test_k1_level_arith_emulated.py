"""The per-level arithmetic of K1 -- the factored patch Hessian (csrc/sia_common.h: sia_patch_hessian, its three S values masked
by membership) and the packed template of a level (sia_ref_tile_packed) -- through the host-emulated library in both widths of
K1 (emu_build.BUILDS 0 and 2), on the frames of tests/k1_level_arith_cases.py, against the oracle with the bounds of
tests/test_sparse_align_emulated.py: poses to 1e-5 in SE(3) log-norm, tracked counts identical, H to 1e-4 of its largest entry.
(The emulation has no frame split over several workgroups: the 600-patch frame runs on the 1024-lane workgroup here and
through the split kernel in tests/test_k1_level_arith_gpu.py.)"""
import numpy as np
import pytest

import k1_level_arith_cases as cases
from rpg_svo_amd import se3
from test_sparse_align_emulated import K1_BUILD_IDS, K1_BUILDS, run_emulated


@pytest.fixture(scope="module", params=K1_BUILDS, ids=K1_BUILD_IDS)
def emu(request):
    from emu_build import BUILDS, build_emulated
    return build_emulated(BUILDS[request.param])


@pytest.fixture(scope="module")
def emu_default():
    from emu_build import build_emulated
    return build_emulated(())


@pytest.mark.parametrize("name", list(cases.WORKGROUP_CASES))
def test_emulated_frames_for_the_level_arithmetic(emu, oracle, name):
    b, (hi, lo, n_iter), T_o, res_o = cases.reference(oracle, name)
    T_h, n_tracked, iters, H, status = run_emulated(emu, b, hi, lo, n_iter=n_iter)
    d = se3.log_norm(T_h, T_o)
    ntr_o = np.array([r["n_tracked"] for r in res_o])
    Ho = np.array([np.asarray(r["H"]).ravel() for r in res_o])
    print(f"{name}: SE3 log-norm to the oracle {d}, n_tracked {n_tracked.tolist()}, "
          f"H off by {np.abs(H - Ho).max() / np.abs(Ho).max():.2e} of the largest entry")
    assert np.all(np.isfinite(T_h))
    # A single patch leaves H with rank 2: the answer then hangs on the rounding inside the solve (the kernels' unpivoted one,
    # Eigen's pivoted LDLT), as tests/test_sparse_align_gpu.py::test_ragged_and_missing_points says; it is counted, not compared.
    posed = b.n >= 8
    assert d[posed].max() <= 1e-5, d
    assert np.array_equal(n_tracked[posed], ntr_o[posed]) and np.all(n_tracked[~posed] <= b.n[~posed])
    assert np.abs(H - Ho)[posed].max() <= 1e-4 * np.abs(Ho).max()


@pytest.mark.parametrize("n_patches", [60, 190])
def test_emulated_wave_kernel_patch_hessian(emu_default, oracle, n_patches):
    """sparse_align_wave.hip calls the helper with T = float, once per patch of a lane (one and three patches per lane): the
    bounds of tests/test_sparse_align_emulated.py::test_emulated_wave_per_frame_kernel"""
    b, (hi, lo, n_iter), T_o, res_o = cases.reference(oracle, "wave", n_patches)
    T_w, ntr_w, it_w, H_w, st_w = run_emulated(emu_default, b, hi, lo, n_iter=n_iter, entry="emu_sparse_align_wave")
    d = se3.log_norm(T_w, T_o)
    print(f"wave kernel, {n_patches} patches: SE3 log-norm to the oracle {d}")
    assert np.all(np.isfinite(T_w))
    assert d.max() <= 1e-4 and np.median(d) <= 1e-5, d
    it_o = np.array([r["iters"][:4] for r in res_o])
    same = np.all(it_o == it_w[:, :4], axis=1)
    assert (~same).sum() <= 1, (it_w[:, :4], it_o)
    assert np.array_equal(ntr_w[same], np.array([r["n_tracked"] for r in res_o])[same])
    Ho = np.array([np.asarray(r["H"]).ravel() for r in res_o])
    assert np.abs(H_w - Ho)[same].max() <= 1e-4 * np.abs(Ho).max()
