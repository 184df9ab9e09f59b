"""The checker of K11 (tests/frame_close_checker.py) against the reference itself (CPU; skipped where the reference checkout
is absent).  tests/host/ref_frame_close.cpp is compiled into build/ref_frame_close/ against oracle/shim together with the
reference's frame.cpp, point.cpp, config.cpp, feature_detection.cpp and map.cpp, where they lie; it builds a Frame whose
fts_ has features with and without a point, in row order, and calls Frame::setKeyframe(), frame_utils::getSceneDepth and
AbstractDetector::setExistingFeatures; and it fills a Map with keyframes and calls Map::getFurthestKeyframe.  Key points,
depth_mean, depth_min and occupancy of every sequence of tests/frame_close_cases.py without out-of-grid pixels, and the
furthest keyframe of every sequence, must equal the checker's bit for bit.

needNewKf and setTrackingQuality are members of FrameHandlerMono / FrameHandlerBase, whose translation units
(frame_handler_mono.cpp, frame_handler_base.cpp) the shims do not carry: in the checker they stay restated from their lines
(frame_handler_mono.cpp:304-315, frame_handler_base.cpp:157-171) and are not pinned here.

Measured: 0 differences over the 30 batches without out-of-grid pixels; the furthest keyframe over all 34."""
import ctypes as C
import os

import numpy as np
import pytest

import frame_close_cases as cases
import frame_close_checker as chk
from first_map_checker import frame_pos, se3_from_Rt
from host_buffers import same_bits
from oracle.pytrack import build_ref_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_UNITS = ("frame", "point", "config", "feature_detection", "map")


@pytest.fixture(scope="module")
def ref():
    lib_path = build_ref_harness(os.path.join(ROOT, "tests", "host", "ref_frame_close.cpp"), REF_UNITS, "ref_frame_close")
    if lib_path is None:
        pytest.skip("no reference checkout to compile frame.cpp / feature_detection.cpp / map.cpp from")
    lib = C.CDLL(lib_path)
    lib.ref_frame_close.restype = C.c_int
    lib.ref_frame_close.argtypes = [C.c_int, C.c_int] + [C.c_double] * 4 + [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 3
    lib.ref_furthest_keyframe.restype = C.c_int
    lib.ref_furthest_keyframe.argtypes = [C.c_int, C.c_int] + [C.c_double] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
    return lib


def cam_args(cam):
    return cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy


def run_reference(ref, cam, T, n, px, f, pos, has_point, grid):
    """-> (return value, key_pts [5], (depth_mean, depth_min), occupancy)"""
    cell_size, n_cols, n_rows = grid
    px, f, T = (np.ascontiguousarray(a, np.float64) for a in (px, f, T))
    pos = np.ascontiguousarray(np.nan_to_num(pos), np.float64)      # (rows without a point: never read)
    hp = np.ascontiguousarray(has_point, np.uint8)
    key_pts, scene, occ = np.full(5, 77, np.int32), np.zeros(2), np.full(n_cols * n_rows, 9, np.uint8)
    rc = ref.ref_frame_close(*cam_args(cam), T.ctypes.data, n, px.ctypes.data, f.ctypes.data, pos.ctypes.data, hp.ctypes.data, cell_size,
                             n_cols * n_rows, key_pts.ctypes.data, scene.ctypes.data, occ.ctypes.data)
    return rc, key_pts, scene, occ


@pytest.mark.parametrize("name", [n for n in cases.NAMES if not n.startswith("bad_pixels")])
def test_checker_has_the_references_bits(ref, name):
    b = cases.batches()[name]
    e = b.expect
    for i, s in enumerate(b.seqs):
        n = min(max(int(s.n), 0), b.n_stride)
        m = int(e["nobs_out"][i])
        rc, key_pts, scene, occ = run_reference(ref, b.cam, e["T_out"][i], n, s.px[:n], s.f[:n], s.pos[:n], s.has_point[:n], b.grid)
        assert rc == (1 if m else 0), (name, i, rc)
        assert np.array_equal(key_pts, e["key_pts"][i]), (name, i, key_pts, e["key_pts"][i])
        assert np.array_equal(occ, e["occupancy"][i]), (name, i)
        if m:   # (the reference leaves the mean unset without a point; the library defines 0, 0)
            assert same_bits(scene, np.array([e["depth_mean"][i], e["depth_min"][i]])), (name, i, scene)


@pytest.mark.parametrize("name", cases.NAMES)
def test_furthest_keyframe_is_the_references(ref, name):
    b = cases.batches()[name]
    for i, s in enumerate(b.seqs):
        n_kf = min(max(int(s.n_kf), 0), b.kf_stride)
        kf_T = np.ascontiguousarray(s.kf_T[:n_kf], np.float64)
        T = np.ascontiguousarray(b.expect["T_out"][i], np.float64)
        got = ref.ref_furthest_keyframe(*cam_args(b.cam), n_kf, kf_T.ctypes.data, T.ctypes.data)
        want = chk.furthest_keyframe([frame_pos(se3_from_Rt(k)) for k in kf_T], frame_pos(se3_from_Rt(T)))
        assert got == want, (name, i, got, want)
        p = dict(chk.DEFAULTS, **b.params)
        if p["max_n_kfs"] > 2 and n_kf >= p["max_n_kfs"]:
            assert b.expect["kf_remove"][i] == got, (name, i)
        else:
            assert b.expect["kf_remove"][i] == -1, (name, i)
