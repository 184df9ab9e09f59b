"""Rows a11 and a13 without a GPU: svo_hip_pose_optimize (the wave kernel, its hand-over to the ordered kernel, the
deferred entry), svo_hip_pose_optimize_ordered and svo_hip_point_optimize of the host-emulated library (tests/emu_build.py:
pose_optimizer_wave.hip, pose_optimizer.hip, point_optimizer.hip compiled for the CPU through tests/host/hip_emu.h) against
the oracle's pose_optimizer::optimizeGaussNewton and Point::optimize, with the requirements of tests/test_tracking_gpu.py
(tests/tracking_cases.py), through tests/tracking_emulated.py."""
import pytest

import tracking_cases as tc
import tracking_emulated as te
from oracle import pytrack


@pytest.fixture(scope="module", params=[0], ids=["default"])
def emu(request):
    from emu_build import build_emulated
    from emu_build import BUILDS
    return build_emulated(BUILDS[request.param])


@pytest.fixture(scope="module")
def emu_default():
    """(the default build only: tests of kernels no queued flag touches)"""
    from emu_build import build_emulated
    return build_emulated(())


@pytest.fixture(scope="module", params=["pinhole", "atan"])
def case(request):
    return tc.committed(request.param)


@pytest.mark.parametrize("ordered,row", [(True, 0), (False, 250), (False, 128), (False, 64)], ids=["ordered", "wave", "wave_rows_of_128", "wave_rows_of_64"])
def test_emulated_pose_optimize(emu, oracle, case, ordered, row):
    batch, want = case.pose_ref("orc", ordered, row)
    got = te.pose_optimize(emu, case.scene.cam, batch, 10, "_ordered" if ordered else "")
    tc.check_pose_batch(case.scene, batch, want, got, ordered)


def test_emulated_pose_optimize_deferred(emu, case):
    batch = tc.pose_deferred_batch(case.scene)
    tc.check_pose_deferred(batch, lambda n_iter, entry: te.pose_optimize(emu, case.scene.cam, batch, n_iter, entry))


def test_emulated_point_optimize(emu_default, oracle, case):
    scene = case.scene
    obs_ptr, fr, ff, p0 = tc.point_optimize_inputs(scene)
    tc.check_point_optimize(pytrack.Track("orc"), scene, obs_ptr, ff, p0, te.point_optimize(emu_default, scene.T_f_w, obs_ptr, fr, ff, p0))


def test_emulated_reproject_points(emu_default, oracle, case):
    tc.check_reproject_points(pytrack.Track("orc"), case.scene, *te.reproject_points(emu_default, case.scene))
