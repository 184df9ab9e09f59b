"""svo_hip_find_match_direct, svo_hip_find_epipolar_match_direct and svo_hip_update_seeds* of the host-emulated build
(tests/emu_build.py) on the cases of tests/track_edge_cases.py: feature and search levels 0 to 4 on both sides of each
other (L), the gather path of the affine warp (Z), features and projections at and beyond the borders with the clamped
source box, warp_sample<true> and the all-zero patch (B), epipolar lines from under two pixels to beyond the cap of 1000
steps through every bucket of the scan's counting sort, with the box per half group on the ATAN camera (E) -- against
the checker by the rules of tests/tracking_cases.py, through tests/tracking_emulated.py.  The coverage
conditions are asserted by track_edge_cases.assert_coverage on the checker and the classifier alone.

Mutations of the emulated build (each run once, on a scratch copy):
  * warp_group.h, xlo = max(..., 0) -> max(..., 1): NO test fails, and none can: xlo enters the results only as the tile
    column xlo & ~15 (the same for 0 and 1), as the address of the dummy read of a sample outside the image, and in the
    emptiness test xhi < xlo, which differs only for xhi == 0, where every sample is outside anyway.  The same change to
    the row, ylo = max(..., 0) -> max(..., 1), fails all twelve tests of case B.
  * depth_filter.hip, SCAN_BUCKETS - 1 -> 3 in the bucket expression: no result changes (45 tests pass) -- the order of
    the scan is performance only, so no test here can notice a wrong bucket.
  * epi_scan.h, `whole` forced to false: no result changes (the scan unit tests and case E pass);
    `boxed` forced to true: tests/test_scan_emulated.py's distorted-camera test aborts in its per-lane class (the box is
    written past the group's block)."""
import pytest

import track_edge_cases as cases
import tracking_cases as tc
import tracking_emulated as te
from oracle import pytrack

CAMS = ("pinhole", "atan", "radtan")
GROUPS = tuple(cases.COVERAGE)
NAMES = tuple(n for g in GROUPS for n in cases.COVERAGE[g][0])


@pytest.fixture(scope="module")
def emu():
    from emu_build import BUILDS, build_emulated
    return build_emulated(BUILDS[0])


@pytest.fixture(scope="module", params=[0, 1], ids=["default", "lane_kernel_with_finish"])
def emu_seeds(request):
    from emu_build import BUILDS, build_emulated
    return build_emulated(BUILDS[request.param])


@pytest.mark.parametrize("cam_kind", CAMS)
@pytest.mark.parametrize("group", GROUPS)
def test_coverage(oracle, group, cam_kind):
    """the classes a group of cases exists for are reached, by the checker's and the classifier's account"""
    cases.assert_coverage(group, cam_kind)


@pytest.mark.parametrize("cam_kind", CAMS)
@pytest.mark.parametrize("name", NAMES)
def test_find_match_direct(emu, oracle, name, cam_kind):
    c = cases.case(name, cam_kind)
    worst = tc.verify_matcher(c, *te.find_match_direct(emu, c))
    print(f"{name} {cam_kind}: max |dA_cur_ref| {worst:.2e}")


@pytest.mark.parametrize("cam_kind", CAMS)
@pytest.mark.parametrize("name", NAMES)
def test_find_epipolar_match_direct(emu, oracle, name, cam_kind):
    c = cases.case(name, cam_kind)
    runs = [(0, 1000), (1, 1000)] + ([(0, c.cap)] if c.cap else [])
    for align_1d, cap in runs:
        wpx, wd = tc.verify_epipolar(c, align_1d, cap, *te.find_epipolar(emu, c, c.epi, align_1d, cap))
        print(f"{name} {cam_kind} align_1d={align_1d} cap={cap}: max |dpx_cur| {wpx:.2e}, max relative depth difference {wd:.2e}")
    if c.cap:   # the smaller cap really fired
        free, capped = c.epi_ref("orc", 0, 1000), c.epi_ref("orc", 0, c.cap)
        assert sum(1 for a, b in zip(free, capped) if a[0] and not b[0]) >= cases.MIN_REJECTED


@pytest.mark.parametrize("cam_kind", CAMS)
@pytest.mark.parametrize("name", NAMES)
def test_update_seeds(emu_seeds, oracle, name, cam_kind):
    c = cases.case(name, cam_kind)
    runs = [(0, 1, 1000)] + ([(0, 0, 1000), (0, 1, c.cap)] if c.cap else [])
    for align_1d, subpix, cap in runs:
        w = tc.verify_seeds(c, align_1d, subpix, cap, *te.update_seeds(emu_seeds, c, align_1d, subpix, cap))
        print(f"{name} {cam_kind} align_1d={align_1d} subpix={subpix} cap={cap}: max deviations {tc.format_deviations(w)}")
    if c.cap:
        free, capped = c.seeds_ref("orc", 0, 1, 1000)[1], c.seeds_ref("orc", 0, 1, c.cap)[1]
        assert sum(1 for a, b in zip(free, capped) if a.status in tc.OK_SEED and b.status == pytrack.SEED_NO_MATCH) >= cases.MIN_REJECTED
