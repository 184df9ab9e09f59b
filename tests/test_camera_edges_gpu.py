"""svo_hip_cam2world, svo_hip_reproject_points and the two camera constructors on the device, where the camera models branch:
the cases of tests/camera_cases.py -- the cases of tests/test_camera_edges_emulated.py, here with the device's tan / atan /
sqrt / division and the real cast_int -- through rpg_svo_amd.tracking and capi, under the same rules, against the mpmath
reference of tests/camera_reference.py and nothing else: no oracle, no reference build.

The bounds (bearings 1e-12, pixels 1e-10 + 1e-13 |px|) leave room for the device's libm: a few ulp times a condition number of
at most 3 (the ATAN corner, dist_r s = 1.15 rad) is about 4e-15 relative.  Every test prints the share of its bound it used.

All cameras go through twelve launches (one of each entry per camera) and one read-back, a few thousand points in all."""
import ctypes as C

import numpy as np
import pytest
import torch

import camera_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def answers(gpu_device):
    """name -> (bearings, cell, px) of every camera's cases"""
    from rpg_svo_amd.tracking import FrameTable, cam2world, reproject_points
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=gpu_device)
    frames = FrameTable(torch.arange(len(cc.FRAMES), dtype=torch.int32, device=gpu_device), t(cc.FRAMES, torch.float64))
    out = {}
    for name in cc.CAMERA_NAMES:
        cam = cc.cameras()[name]
        _, frame, pos, _ = cc.points(name)
        f = cam2world(cam, t(cc.pixels(name)[1], torch.float64))
        cell = torch.full((len(pos),), -7, dtype=torch.int32, device=gpu_device)
        px = torch.full((len(pos), 2), float("nan"), dtype=torch.float64, device=gpu_device)
        reproject_points(cam, frames, t(frame, torch.int32), t(pos, torch.float64), cc.CELL, cc.n_cols(cam), out=(cell, px))
        out[name] = (f, cell, px)
    torch.cuda.synchronize()
    return {k: tuple(x.cpu().numpy() for x in v) for k, v in out.items()}


@pytest.mark.parametrize("name", cc.CAMERA_NAMES)
def test_bearings_against_the_reference(answers, name):
    print(name, "largest bearing error:", cc.check_bearings(name, answers[name][0]), "of", cc.BEARING_TOL)


@pytest.mark.parametrize("name", cc.CAMERA_NAMES)
def test_reprojections_against_the_reference(answers, name):
    _, cell, px = answers[name]
    print(name, "largest share of the pixel bound used:", cc.check_pixels(name, px))
    cc.check_cells(name, cell)


def test_constructors(hip_lib):
    from rpg_svo_amd import capi
    for args in cc.PINHOLE_CTOR_ARGS:
        out = capi.Camera()
        capi.check(hip_lib.svo_hip_camera_pinhole(*args, C.byref(out)), "svo_hip_camera_pinhole")
        cc.check_constructor("pinhole", args, out)
    for args in cc.ATAN_CTOR_ARGS:
        out = capi.Camera()
        capi.check(hip_lib.svo_hip_camera_atan(*args, C.byref(out)), "svo_hip_camera_atan")
        cc.check_constructor("atan", args, out)
        # capi.camera of the cases' description (what every kernel above received) is the struct the constructor makes
        want = capi.camera(cc.cameras()["atan" if args[6] else "atan_s0"])
        for k in ("fx", "fy", "cx", "cy", "width", "height", "model"):
            assert getattr(out, k) == getattr(want, k), k
        assert list(out.d) == list(want.d)
