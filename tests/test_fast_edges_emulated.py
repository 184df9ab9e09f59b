"""svo_hip_fast_detect (K7) of the host-emulated library on the cases of tests/fast_cases.py: S slots, T ties, B borders, P the
full cross of the two thresholds, C shapes, E empty cells under a threshold that rounds up in float -- each bit for bit
against the oracle, the designed images (T, B, C) also against the independent detector of tests/fast_reference.py, and the
reference's own detector where oracle/_ref is built.  (G, the second launch pass, needs 10^7 fibers: device only.)"""
import numpy as np
import pytest

import fast_cases as fc
import first_map_checker as chk
from test_fast_emulated import detect
from test_first_map_emulated import call_seeds


@pytest.fixture(scope="module")
def emu():
    from emu_build import build_emulated
    return build_emulated((), bind=("svo_hip_first_map", "svo_hip_initialize_seeds"))   # (call_seeds passes addresses as ints)


def run(emu, c):
    """the emulated backend: -> xy, level, score [n, cells(, 2)]"""
    return detect(emu, c.images, c.n_pyr, c.n_levels, c.cell, c.occ, thresh=c.thresh, slots=c.slots, fast_threshold=c.fast_threshold,
                  n_store_slots=c.n_store_slots, image_slots=c.image_slots)[:3]


def test_slots(emu, oracle):
    c = fc.case_slots()
    got = run(emu, c)
    fc.verify(c, got)
    fc.verify_ref_leg(c, got)


@pytest.mark.parametrize("n_levels", [1, 2])
def test_ties(emu, oracle, n_levels):
    c = fc.case_ties(n_levels)
    got = run(emu, c)
    fc.verify(c, got)
    fc.verify_reference(c, got)
    fc.verify_ref_leg(c, got)


@pytest.mark.parametrize("doubled", [False, True])
@pytest.mark.parametrize("fast_threshold", [20, 254])
def test_borders(emu, oracle, fast_threshold, doubled):
    c = fc.case_borders(fast_threshold, doubled)
    got = run(emu, c)
    fc.verify(c, got)
    fc.verify_reference(c, got)
    fc.verify_ref_leg(c, got)


@pytest.mark.parametrize("fast_threshold,thresh", fc.P_CROSS)
def test_parameters(emu, oracle, fast_threshold, thresh):
    c = fc.case_parameters(fast_threshold, thresh)
    got = run(emu, c)
    fc.verify(c, got)
    fc.verify_ref_leg(c, got)


@pytest.mark.parametrize("w,h,levels,cell", fc.SHAPES)
def test_shapes(emu, oracle, w, h, levels, cell):
    c = fc.case_shape(w, h, levels, cell)
    got = run(emu, c)
    fc.verify(c, got)
    fc.verify_reference(c, got)


@pytest.mark.parametrize("occupied", [True, False])
@pytest.mark.parametrize("thresh", fc.E_THRESHOLDS)
def test_empty_cells_become_no_seed(emu, oracle, thresh, occupied):
    """detect -> initialize_seeds: a cell is a seed iff level >= 0, also where float(threshold) > threshold and the empty and the
    occupied cells' scores pass "score > threshold" (the oracle, faithful to the reference, counts all six cells there)"""
    import types
    c = fc.case_empty(thresh, occupied)
    xy, lvl, sc = run(emu, c)
    fc.verify(c, (xy, lvl, sc))
    fc.verify_ref_leg(c, (xy, lvl, sc))
    n_corners = int((lvl[0] >= 0).sum())
    cam = types.SimpleNamespace(width=c.w, height=c.h, fx=80.0, fy=80.0, cx=44.5, cy=29.5, model=0, d=(0.0,) * 5)
    s = types.SimpleNamespace(n_frames=1, n_cells=c.n_cells, threshold=thresh, cam=cam, xy=xy, level=lvl, score=sc,
                              frame_index=np.array([7], np.int32), depth_mean=np.array([2.0]), depth_min=np.array([0.5]))
    rc, out = call_seeds(emu, s, c.n_cells, 1)
    assert rc == 0 and out.guards_intact()
    assert out.view["n_seeds"][0] == n_corners == (3 if occupied else 4)
    assert (out.view["level"][0, :n_corners] >= 0).all() and (out.view["px"][0, :n_corners] >= 0).all()
    assert np.array_equal(out.view["px"][0, :n_corners], xy[0][lvl[0] >= 0].astype(np.float64))
    want = chk.initialize_seeds(cam, xy, lvl, sc, thresh, s.frame_index, s.depth_mean, s.depth_min, 1, c.n_cells)
    assert want["n_seeds"][0] == n_corners
