"""K1 -- the headline kernel -- without a GPU: rpg_svo_amd/csrc/sparse_align.hip in the host-emulated library
(tests/k1_emulated.py, tests/emu_build.py) on the cases of tests/k1_cases.py, in both widths of K1, against the oracle's
SparseImgAlign::run under the emulated profiles of that module's rule: poses to 1e-5 in SE(3) log-norm on the base and edge
cases and to 1e-4 elsewhere, tracked counts identical, H to 1e-4 of its largest entry, at most one frame with another
iteration sequence.  What a test asserts beyond the rule is what its case is for."""
import numpy as np
import pytest

import k1_cases as k1
import k1_emulated
from rpg_svo_amd import se3


@pytest.fixture(scope="module", params=k1_emulated.K1_BUILDS, ids=k1_emulated.K1_BUILD_IDS)
def emu(request):
    """both widths of K1: every test that takes `emu` holds its bounds on each"""
    return k1_emulated.Emulated(request.param)


@pytest.fixture(scope="module")
def emu_default():
    """(the default build only: the wave-per-frame kernel reads no width flag)"""
    return k1_emulated.Emulated(0)


def run_and_verify(emu, oracle, name, schedule=None, kernel="auto"):
    """-> (the case, the backend's answer, what the rule measured)"""
    c = k1.case(name)
    schedule = schedule or c.schedules[0]
    answer = emu.run(c, schedule, kernel)
    return c, answer, k1.verify_pair(oracle, emu.backend(kernel), name, schedule, answer)


def test_emulated_sparse_align_follows_the_oracle(emu, oracle):
    c, answer, m = run_and_verify(emu, oracle, "vga16")
    assert se3.log_norm(answer.pose, c.batch.T_gt_w[:6]).max() < 5e-3      # and the motion is recovered


def test_emulated_sparse_align_edge_cases(emu, oracle):
    """ragged feature counts, features without a point, an empty frame (pose untouched, nothing tracked), the reference's
    default schedule (levels 4 -> 2 of a 5-level pyramid)"""
    c, answer, m = run_and_verify(emu, oracle, "edge")
    assert answer.n_tracked[2] == 0
    assert np.abs(answer.pose[2] - c.batch.T_cur_w[2]).max() < 1e-12  # (the prior, up to the product T_cur_ref * T_ref)


def test_emulated_ragged_and_missing_points(emu, oracle):
    """n = 200, 12, 64, 65, 137, 0, 1 with holes: the device's ragged case under AddressSanitizer's eyes
    (scripts/emu_sanitize.sh runs this file)"""
    k1.verify_ragged(oracle, emu.name, emu.run(k1.case("ragged"), k1.case("ragged").schedules[0]))


@pytest.mark.parametrize("n_patches", [60, 190])
def test_emulated_wave_per_frame_kernel(emu_default, oracle, n_patches):
    """sparse_align_wave.hip -- a frame per wave, one and three patches per lane, no workgroup barrier, the solve in the same
    wave behind a transposing wave reduction -- through its test-only entry: the oracle's poses, and the workgroup kernel's"""
    name = f"wave_{n_patches}"
    c, wave, m = run_and_verify(emu_default, oracle, name, kernel="wave")
    workgroup = emu_default.run(c, c.schedules[0])
    assert se3.log_norm(wave.pose, workgroup.pose).max() <= 1e-4


@pytest.mark.parametrize("kind", ["radtan", "atan"])
def test_emulated_distorted_camera_models(emu, oracle, kind):
    """the DIST instantiation of sia_kernel (the camera model's world2cam in the loop, no window cache) -- and, for 60 patches
    per frame, of the wave-per-frame kernel: the oracle's poses through the vikit models' projection"""
    name, schedule = f"{kind}_60", (4, 2, 30)
    c, workgroup, m = run_and_verify(emu, oracle, name, schedule)
    c, wave, m = run_and_verify(emu, oracle, name, schedule, kernel="wave")
    assert se3.log_norm(wave.pose, workgroup.pose).max() <= 1e-4
    assert se3.log_norm(workgroup.pose, c.batch.T_gt_w[:3]).max() < 5e-3   # both solved the problem (60 patches, levels 4 -> 2)


def test_emulated_border_features_outside_patches_and_iteration_caps(emu, oracle):
    """features in the 3..30 px band next to a border (invisible at coarse levels, joining at finer ones: the H rebuild when
    the set of patches inside the image changes); a prior so wrong that nothing projects into the image (H = 0, x = 0, the
    pose kept); n_iter = 0, 1, 2"""
    for schedule in k1.case("border").schedules:   # the full schedule (every feature joins eventually) and a stop at level 2 (some never do)
        c, answer, m = run_and_verify(emu, oracle, "border", schedule)
    assert np.all(answer.n_tracked < 200) and np.all(answer.n_tracked > 100), answer.n_tracked
    k1.verify_outside(oracle, emu.name, "border_outside", emu.run(k1.case("border_outside"), k1.case("border_outside").schedules[0]))
    for schedule in k1.ITERATION_CAP_SCHEDULES:
        run_and_verify(emu, oracle, "border_itercap", schedule)


@pytest.mark.parametrize("level", [3, 0])
def test_emulated_single_gauss_newton_step(emu, oracle, level):
    """One Gauss-Newton step, one level (n_iter = 1, max_level = min_level), 12 VGA frames of 200 patches, from a prior that is
    5e-3 off in rotation and translation alike.  The loops of the other tests correct themselves: an error of first order in
    the update -- SE3::exp of the reference-width build, a product of the Jacobian rows -- is gone an iteration later and only
    moves an iteration count.  Here the pose IS the update, and such an error of about |rotation| x |translation| / 2 ~ 1e-5 of
    the step stands two orders above the bound (k1_cases.SINGLE_STEP_BOUND, with the figures it comes from)."""
    c, answer, m = run_and_verify(emu, oracle, f"step_level{level}")
    T_o, _ = k1.reference(oracle, c.name, c.schedules[0])
    step = se3.log_norm(T_o, c.batch.T_cur_w)
    print(f"single step at level {level}: max distance to the oracle {m.d.max():.3e}, step sizes {step.min():.2e} .. {step.max():.2e}")
    assert answer.iters[:, level].tolist() == [1] * 12
    assert step.min() > 1e-3                       # (a step with something to get wrong)
