"""The per-level arithmetic of K1 on the device -- the factored patch Hessian of both K1 kernels and the packed template of the
256-lane workgroup kernel (csrc/sia_common.h) -- on the frames of tests/k1_level_arith_cases.py against the oracle, with the
bounds of tests/test_sparse_align_gpu.py: poses to 1e-4 in SE(3) log-norm, and on frames that ran the oracle's iteration counts
the tracked counts identical and H to rtol 1e-5 plus 1e-3 of its largest entry.  The 600-patch frame takes the kernel split
over four workgroups here; a radtan and an atan camera cover the DIST instantiations; a frame aligned against itself must come
out with a chi2 of exactly zero, level by level (template and warped patch round alike)."""
import numpy as np
import pytest

import k1_level_arith_cases as cases
from helpers import run_hip, tile_batch
from rpg_svo_amd import se3

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _against_the_oracle(b, sched, T_o, res_o, T_h, out, what, rows=slice(None), h_rtol=1e-5):
    d = se3.log_norm(T_h[rows], T_o)
    it_o = np.array([r["iters"] for r in res_o])
    same = np.all(it_o == out.iters.cpu().numpy()[rows], axis=1)
    ntr_o = np.array([r["n_tracked"] for r in res_o])
    ntr = out.n_tracked.cpu().numpy()[rows]
    Ho = np.stack([r["H"] for r in res_o]).reshape(-1, 36)
    Hh = out.H.cpu().numpy().reshape(-1, 36)[rows]
    # (a single patch leaves H with rank 2 and the pose to the rounding of the solve: test_ragged_and_missing_points)
    posed = b.n >= 8
    print(f"{what}: SE3 log-norm to the oracle {d}, same iteration counts {same.tolist()}, "
          f"H off by {np.abs(Hh - Ho)[same & posed].max() / np.abs(Ho).max():.2e} of the largest entry")
    assert np.all(np.isfinite(T_h))
    assert d[posed].max() <= TOL, d
    assert (~same[posed]).sum() <= 1, (it_o, out.iters.cpu().numpy()[rows])
    ok = same & posed
    assert np.array_equal(ntr[ok], ntr_o[ok]) and np.all(ntr[~posed] <= b.n[~posed])
    assert np.allclose(Hh[ok], Ho[ok], rtol=h_rtol, atol=1e-3 * np.abs(Ho).max())


@pytest.mark.parametrize("name", list(cases.WORKGROUP_CASES))
def test_frames_for_the_level_arithmetic(oracle, gpu_device, name):
    b, (hi, lo, n_iter), T_o, res_o = cases.reference(oracle, name)
    T_h, out, _ = run_hip(b, hi, lo, n_iter)
    _against_the_oracle(b, (hi, lo, n_iter), T_o, res_o, T_h, out, name)


@pytest.mark.parametrize("n", [64, 200])
@pytest.mark.parametrize("kind", ["radtan", "atan"])
def test_distorted_cameras(oracle, gpu_device, kind, n):
    b, (hi, lo, n_iter), T_o, res_o = cases.reference(oracle, "distorted", kind, n)
    T_h, out, _ = run_hip(b, hi, lo, n_iter)
    _against_the_oracle(b, (hi, lo, n_iter), T_o, res_o, T_h, out, f"{kind}, {n} patches")
    assert se3.log_norm(T_h, b.T_gt_w).max() < 5e-3   # the problem was solved (levels 4 -> 2 only)


@pytest.mark.parametrize("n_patches", [60, 190])
def test_wave_kernel_patch_hessian(oracle, gpu_device, n_patches):
    """the wave-per-frame kernel (batches of >= 1024 frames): H accumulated in f32, the bound of
    tests/test_sparse_align_gpu.py::test_wave_per_frame_kernel (rtol 2e-5)"""
    b, (hi, lo, n_iter), T_o, res_o = cases.reference(oracle, "wave", n_patches)
    T_w, out_w, _ = run_hip(tile_batch(b, 256), hi, lo, n_iter, kernel="auto")
    assert np.array_equal(T_w.reshape(256, 4, 12), np.broadcast_to(T_w[:4], (256, 4, 12)))
    _against_the_oracle(b, (hi, lo, n_iter), T_o, res_o, T_w, out_w, f"wave kernel, {n_patches} patches", rows=slice(0, 4), h_rtol=2e-5)


def test_self_aligned_frames_have_zero_residuals(gpu_device):
    b, (hi, lo, n_iter) = cases.case("self_aligned")[:2]
    for top, bottom in [(hi, lo)] + [(l, l) for l in range(lo, hi + 1)]:
        T_h, out, _ = run_hip(b, top, bottom, n_iter)
        chi2 = out.chi2.cpu().numpy()
        print(f"levels {top} -> {bottom}: chi2 {chi2}, SE3 log-norm to the prior {se3.log_norm(T_h, b.T_ref_w)}")
        assert np.array_equal(chi2, np.zeros_like(chi2)), chi2
        assert np.all(out.n_tracked.cpu().numpy() >= b.n - 20)   # (all but the patches 3 px from the border of the top level)
        assert se3.log_norm(T_h, b.T_ref_w).max() < 1e-7
