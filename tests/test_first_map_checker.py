"""The checker of K10 (tests/first_map_checker.py) against the reference itself (CPU; skipped where the reference checkout
is absent).  tests/host/ref_first_map.cpp is compiled into build/ref_first_map/ against oracle/shim together with the
reference's frame.cpp, point.cpp, config.cpp and feature_detection.cpp, where they lie; it builds two Frames, adds the
Point / Feature pairs in rank order and calls Frame::setKeyframe(), frame_utils::getSceneDepth and
AbstractDetector::setExistingFeatures.  Key points, occupancy, depth_mean and depth_min of every sequence of
tests/first_map_cases.py must equal the checker's bit for bit.  The cases with pixels outside the grid are left to the
stated differences: there the reference's .at() throws, or a column beyond the grid wraps into the next row (the last test
shows both).  A Seed's fields are the oracle's seed_init, which tests/test_oracle_vs_ref.py pins to the reference; where
the reference library of oracle/ is built they are compared with its Seed constructor here as well.

Measured: 0 differences over the 28 batches (88 sequences, 11 of them without SUCCESS or without a point), all four cameras."""
import ctypes as C
import os

import numpy as np
import pytest

import first_map_cases as cases
import first_map_checker as chk
from host_buffers import same_bits
from oracle.pytrack import build_ref_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_UNITS = ("frame", "point", "config", "feature_detection")


@pytest.fixture(scope="module")
def ref():
    lib_path = build_ref_harness(os.path.join(ROOT, "tests", "host", "ref_first_map.cpp"), REF_UNITS, "ref_first_map")
    if lib_path is None:
        pytest.skip("no reference checkout to compile frame.cpp / feature_detection.cpp from")
    lib = C.CDLL(lib_path)
    lib.ref_first_map.restype = C.c_int
    lib.ref_first_map.argtypes = [C.c_int, C.c_int] + [C.c_double] * 4 + [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 3
    return lib


def run_reference(ref, cam, T_cur_w, pos, px, f, grid):
    """-> (return value, key_pts [2, 5], (depth_mean, depth_min), occupancy)"""
    cell_size, n_cols, n_rows = grid
    n = len(pos)
    pos, px, f, T = (np.ascontiguousarray(a, np.float64) for a in (pos, px, f, T_cur_w))
    key_pts, scene, occ = np.full((2, 5), 77, np.int32), np.zeros(2), np.full(n_cols * n_rows, 9, np.uint8)
    rc = ref.ref_first_map(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, T.ctypes.data, n, pos.ctypes.data, px.ctypes.data,
                           f.ctypes.data, cell_size, n_cols * n_rows, key_pts.ctypes.data, scene.ctypes.data, occ.ctypes.data)
    return rc, key_pts, scene, occ


@pytest.mark.parametrize("name", [n for n in cases.NAMES if not n.startswith("bad_pixels")])
def test_checker_has_the_references_bits(ref, name):
    b = cases.batches()[name]
    e = b.expect
    for i, s in enumerate(b.seqs):
        if int(s.result) != chk.SUCCESS:
            assert e["n_points"][i] == 0
            continue
        n = int(e["n_points"][i])
        rc, key_pts, scene, occ = run_reference(ref, b.cam, s.T_cur_w, e["pos"][i, :n], e["px"][i, :, :n], e["f"][i, :, :n], b.grid)
        assert rc == (1 if n else 0), (name, i, rc)
        assert np.array_equal(key_pts, e["key_pts"][i]), (name, i, key_pts, e["key_pts"][i])
        assert np.array_equal(occ, e["occupancy"][i]), (name, i)
        if n:   # (the reference leaves both unset without a point; the library defines 0, 0)
            assert same_bits(scene, np.array([e["depth_mean"][i], e["depth_min"][i]])), (name, i, scene)


def test_seed_fields_are_the_reference_constructors():
    from oracle import pytrack
    if not pytrack.ref_available():
        pytest.skip("oracle/_ref/libsvo_ref.so not built (needs the reference checkout at build time)")
    orc, ref_track = pytrack.Track("orc"), pytrack.Track("ref")
    for name in cases.SEED_NAMES:
        c, stride, batch_id = cases.seed_cases()[name]
        for fr in range(c.n_frames):
            a = orc.seed_init(float(np.float32(c.depth_mean[fr])), float(np.float32(c.depth_min[fr])))
            r = ref_track.seed_init(float(np.float32(c.depth_mean[fr])), float(np.float32(c.depth_min[fr])))
            n = int(c.expect["n_seeds"][fr])
            for k in ("a", "b", "mu", "z_range", "sigma2"):
                want = np.float32(getattr(r, k))
                assert same_bits(np.float32(getattr(a, k)), want), (name, fr, k)
                assert all(same_bits(v, want) for v in c.expect[k][fr, :n]), (name, fr, k)


def test_the_stated_differences_outside_the_grid(ref):
    """A pixel whose cell index leaves the grid: the reference's .at() throws; one whose column lies beyond the grid but
    whose index stays inside wraps into the next row.  The library sets no cell in either case."""
    cam, cell = cases.CAMERAS["160x120"]
    grid = cases.grid(cam, cell)
    T = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
    pos, f = np.array([[0.0, 0.0, 2.0]]), np.array([[[0.0, 0.0, 1.0]], [[0.0, 0.0, 1.0]]])
    px = lambda x, y: np.array([[[10.0, 10.0]], [[x, y]]])
    assert run_reference(ref, cam, T, pos, px(10.0, 4000.0), f, grid)[0] == -2
    assert chk.cell_of((10.0, 4000.0), *grid) == -1
    rc, _, _, occ = run_reference(ref, cam, T, pos, px(grid[1] * cell + 5.0, 10.0), f, grid)
    assert rc == 1 and list(np.flatnonzero(occ)) == [grid[1]]                # column n_cols of row 0 is cell 0 of row 1
    assert chk.cell_of((grid[1] * cell + 5.0, 10.0), *grid) == -1
