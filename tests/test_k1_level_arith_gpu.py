"""The per-level arithmetic of K1 on the device -- the factored patch Hessian of both K1 kernels and the packed template of the
256-lane workgroup kernel (csrc/sia_common.h) -- on the frames tests/k1_cases.py builds for it, against the oracle under that
module's rule: poses to 1e-4 in SE(3) log-norm, and on frames that ran the oracle's iteration counts the tracked counts
identical and H to rtol 1e-5 (the wave kernel: 2e-5) plus 1e-3 of its largest entry.  The 600-patch frame takes the kernel split
over four workgroups here; a radtan and an atan camera cover the DIST instantiations; a frame aligned against itself must come
out with a chi2 of exactly zero, level by level (template and warped patch round alike)."""
import numpy as np
import pytest

import k1_cases as k1
import k1_device
from rpg_svo_amd import se3

pytestmark = pytest.mark.gpu


def run_and_verify(oracle, name):
    c = k1.case(name)
    answer = k1_device.run(c, c.schedules[0])
    k1.verify_pair(oracle, k1.DEV, name, c.schedules[0], answer)
    return c, answer


@pytest.mark.parametrize("name", k1.LEVEL_ARITH_FRAMES)
def test_frames_for_the_level_arithmetic(oracle, gpu_device, name):
    run_and_verify(oracle, name)


@pytest.mark.parametrize("n", [64, 200])
@pytest.mark.parametrize("kind", ["radtan", "atan"])
def test_distorted_cameras(oracle, gpu_device, kind, n):
    c, answer = run_and_verify(oracle, f"{kind}_{n}")
    assert se3.log_norm(answer.pose, c.batch.T_gt_w).max() < 5e-3   # the problem was solved (levels 4 -> 2 only)


@pytest.mark.parametrize("n_patches", [60, 190])
def test_wave_kernel_patch_hessian(oracle, gpu_device, n_patches):
    """the wave-per-frame kernel (4 frames, 256 times over: batches of >= 1024 frames): H accumulated in f32"""
    c, answer = run_and_verify(oracle, f"wave_arith_{n_patches}")
    assert np.array_equal(answer.pose.reshape(256, 4, 12), np.broadcast_to(answer.pose[:4], (256, 4, 12)))


def test_self_aligned_frames_have_zero_residuals(gpu_device):
    c = k1.case("self_aligned")
    b, (hi, lo, n_iter) = c.batch, c.schedules[0]
    for top, bottom in [(hi, lo)] + [(l, l) for l in range(lo, hi + 1)]:
        answer = k1_device.run(c, (top, bottom, n_iter))
        print(f"levels {top} -> {bottom}: chi2 {answer.chi2}, SE3 log-norm to the prior {se3.log_norm(answer.pose, b.T_ref_w)}")
        assert np.array_equal(answer.chi2, np.zeros_like(answer.chi2)), answer.chi2
        assert np.all(answer.n_tracked >= b.n - 20)   # (all but the patches 3 px from the border of the top level)
        assert se3.log_norm(answer.pose, b.T_ref_w).max() < 1e-7
