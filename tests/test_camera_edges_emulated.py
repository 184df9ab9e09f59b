"""svo_hip_cam2world and svo_hip_reproject_points where the camera models branch, without a GPU (host-emulated library,
tests/emu_build.py), and the two camera constructors of the C ABI (host code of the product library): every case of
tests/camera_cases.py under its rules against the mpmath reference of tests/camera_reference.py, and -- the emulation runs the
host's libm with contraction off -- equal to the C oracle bit for bit in the bearings and the pixels."""
import ctypes as C

import numpy as np
import pytest

import camera_cases as cc
from host_buffers import ptr
from oracle import pytrack
from rpg_svo_amd import capi


@pytest.fixture(scope="module")
def emu():
    from emu_build import build_emulated
    return build_emulated(())


@pytest.fixture(scope="module")
def host_lib():
    """The constructors are host code of capi_util.hip, which the emulated library leaves out (it wraps the HIP runtime): the
    product library's own are called -- no device is touched, as with the pyramid layout in tests/tracking_emulated.py."""
    return capi.load()


def _answers(emu, name):
    """-> bearings [n,3], cell [m], px [m,2] of the camera's cases: one launch each"""
    cam = cc.cameras()[name]
    cs = capi.camera(cam)
    _, px = cc.pixels(name)
    f = np.full((len(px), 3), np.nan)
    assert emu.svo_hip_cam2world(C.byref(cs), len(px), ptr(np.ascontiguousarray(px)), ptr(f), None) == 0
    _, frame, pos, _ = cc.points(name)
    slots = np.arange(len(cc.FRAMES), dtype=np.int32)
    frames = capi.Frames(len(cc.FRAMES), 0, slots.ctypes.data, cc.FRAMES.ctypes.data)
    cell, out = np.full(len(pos), -7, np.int32), np.full((len(pos), 2), np.nan)
    assert emu.svo_hip_reproject_points(C.byref(cs), C.byref(frames), len(pos), ptr(frame), ptr(pos), cc.CELL, cc.n_cols(cam), ptr(cell), ptr(out),
                                        None) == 0
    return f, cell, out


@pytest.mark.parametrize("name", cc.CAMERA_NAMES)
def test_emulated_cameras_against_the_reference_and_the_oracle(emu, oracle, name):
    f, cell, px = _answers(emu, name)
    cc.check_all(name, f, cell, px)
    cam, orc = cc.cameras()[name], pytrack.Track("orc")
    assert np.array_equal(f, orc.cam2world(cam, cc.pixels(name)[1]))
    _, frame, pos, _ = cc.points(name)
    for i in range(len(pos)):
        k, p = orc.reproject_point(cam, cc.FRAMES[frame[i]], pos[i], cc.CELL, cc.n_cols(cam))
        assert k == cell[i] and np.array_equal(p, px[i], equal_nan=True), (name, i, cc.points(name)[0][i], p, px[i])


@pytest.mark.parametrize("args", cc.PINHOLE_CTOR_ARGS, ids=lambda a: f"d0={a[6]:g}")
def test_pinhole_constructor(host_lib, args):
    """vk::PinholeCamera's switch: fabs(d0) > 1e-7 keeps all five coefficients, anything else zeroes d1..d4 with it"""
    out = capi.Camera()
    out.reserved = 77
    assert host_lib.svo_hip_camera_pinhole(*args, C.byref(out)) == 0
    cc.check_constructor("pinhole", args, out)
    assert out.reserved == 0


@pytest.mark.parametrize("args", cc.ATAN_CTOR_ARGS, ids=lambda a: f"s={a[6]:g}")
def test_atan_constructor(host_lib, args):
    """vk::ATANCamera's normalisation (width fx, cx width - 0.5) and constants; s == 0: no constants, the pinhole"""
    out = capi.Camera()
    assert host_lib.svo_hip_camera_atan(*args, C.byref(out)) == 0
    cc.check_constructor("atan", args, out)
    # and the struct the cases use (rpg_svo_amd.synth.Camera.atan) is the one the constructor makes
    want = capi.camera(cc.cameras()["atan" if args[6] else "atan_s0"])
    assert bytes(out) == bytes(want)
