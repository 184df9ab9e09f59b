"""The rules of tests/fast_cases.py bite: the independent detector of tests/fast_reference.py passes every case, and each of its
named mutants -- one wrong rule each -- is caught by the case that is there for it.  Also: the builders' own asserts (at least
10 tied cells in T, the four survivors of B, parameters that are no no-ops in P, frames 1 and 2 of S that differ), and the
vectorised segment test against the scalar brute force.  CPU only; nothing here loads the library under test."""
import numpy as np
import pytest

import fast_cases as fc
import fast_reference as fr

CASES = {"S": fc.case_slots, "T1": lambda: fc.case_ties(1), "T2": lambda: fc.case_ties(2), "B20": lambda: fc.case_borders(20),
         "B254": lambda: fc.case_borders(254), "B20x2": lambda: fc.case_borders(20, True), "B254x2": lambda: fc.case_borders(254, True),
         "P7/20.0": lambda: fc.case_parameters(7, 20.0), "P60/20.1": lambda: fc.case_parameters(60, 20.1),
         "E20.1": lambda: fc.case_empty(20.1), "E0.1": lambda: fc.case_empty(0.1), "E20.3": lambda: fc.case_empty(20.3), "G": fc.case_second_pass}

# mutant -> the cases that must catch it (the first one is the case named for it)
CAUGHT_BY = {"tie_last_in_raster": ("T1", "T2"),
             "update_greater_equal": ("T1", "T2"),
             "image_at_frame": ("S",),
             "state_by_slot": ("S",),
             "shi_tomasi_border": ("B20", "B254", "B20x2"),
             "fast_threshold_ignored": ("P7/20.0", "P60/20.1"),
             "empty_is_feature": ("E20.1", "E0.1"),
             "second_pass_empty": ("G",)}


def test_every_mutant_has_a_case():
    assert set(CAUGHT_BY) == set(fr.MUTANTS) and len(fr.MUTANTS) == 8


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_independent_detector_passes(oracle, name):
    """(oracle and independent detector agree on every case: pixel, level, score within the f32 tolerance, empty cells)"""
    c = CASES[name]()
    fc.verify_against_oracle_loosely(c, c.reference())
    fc.verify_reference(c, c.expected())
    fc.verify(c, c.expected())


@pytest.mark.parametrize("mutant,name", [(m, n) for m, names in CAUGHT_BY.items() for n in names])
def test_mutant_is_caught(oracle, mutant, name):
    c = CASES[name]()
    got = c.reference(mutant)
    with pytest.raises(AssertionError):
        fc.verify_against_oracle_loosely(c, got)


def test_state_by_slot_shows_on_the_frames_that_share_a_slot(oracle):
    c = fc.case_slots()
    xy, lvl, _ = c.reference("state_by_slot")
    exy, elvl, _ = c.expected()
    assert np.array_equal(lvl[1], lvl[2]) and not np.array_equal(elvl[1], elvl[2])       # the mutant's frames 1 and 2 are one answer
    assert all(np.array_equal(lvl[f], elvl[f]) and np.array_equal(xy[f], exy[f]) for f in (0, 3, 4))   # and nothing else shows it


def test_empty_cells_that_are_no_feature_do_not_catch_at_a_threshold_that_rounds_down(oracle):
    c = fc.case_empty(20.3)
    fc.verify_against_oracle_loosely(c, c.reference("empty_is_feature"))                    # float(20.3) < 20.3: nothing to report


def test_second_pass_mutant_shows_on_the_last_frame_alone(oracle):
    c = fc.case_second_pass()
    _, lvl, _ = c.reference("second_pass_empty")
    _, elvl, _ = c.expected()
    differs = (lvl != elvl).any(axis=1)
    assert differs[-1] and not differs[:-1].any() and c.n == fc.K7_FRAMES_PER_PASS(5) + 1


def test_the_builders_own_asserts(oracle):
    fc.check_parameters_bite()
    for make in CASES.values():
        make()
    for shape in fc.SHAPES:
        fc.case_shape(*shape)
    t = fc.case_ties(1)
    print(f"T: {len(t.candidates(0))} corners, {(t.margins()[0] == 0).sum()} of {t.n_cells} cells tied")
    # the smallest pyramids: no cell of a level that is narrower than 7 pixels holds a corner
    assert (fc.case_shape(1, 1, 1, 1).expected()[1] == -1).all()
    assert all(L == 0 for _, _, _, L, _ in fc.case_shape(13, 12, 2, 4).candidates(0))
    assert fc.P_DIAGONAL == ((1, 0.0), (7, 5.5), (20, 20.0), (60, 20.1), (1, 20.3), (7, 150.0)) and len(fc.P_CROSS) == 24


def test_vectorised_segment_test_is_the_scalar_brute_force():
    """fast_scores (arc minima, one comparison per threshold) against is_corner pixel by pixel and threshold by threshold"""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(24, 28)).astype(np.uint8)
    img[8:18, 6:20] = (img[8:18, 6:20] // 4 + 150).astype(np.uint8)
    S = fr.fast_scores(img, 20)
    n = 0
    for y in range(24):
        for x in range(28):
            inside = 3 <= x < 25 and 3 <= y < 21
            if not (inside and fr.is_corner(img, x, y, 20)):
                assert S[y, x] == -1
                continue
            best = max(t for t in range(20, 255) if fr.is_corner(img, x, y, t))
            assert S[y, x] == best and all(fr.is_corner(img, x, y, t) for t in range(20, best + 1))    # (monotone: bisection finds it, too)
            n += 1
    assert n > 10
