"""tracking.Matcher, tracking.find_epipolar_match_direct and tracking.DepthFilter on the device on the cases of
tests/track_edge_cases.py -- those of tests/test_track_edges_emulated.py, here with the real v_alignbyte, DPP moves, the
hand-overs through LDS inside a wave and fused multiply-adds: feature and search levels 0 to 4 (L), the gather path of the
warp (Z), borders with the clamped box, warp_sample<true> and the all-zero patch (B), lines from under two pixels to beyond
the cap through every bucket of the scan, the box per half group on the ATAN camera, and the resident entry (E).  On all
of CAMERA_KINDS, against both checkers, by the rules of tests/tracking_cases.py (verify_*), through tests/tracking_device.py.
Every test prints its class counts and its largest deviations.

Measured on an MI355X (93 tests, 21 s): every verdict, observation, search level, patch and refined pixel identical in all
cases; largest deviations A_cur_ref 6.8e-14 (L05, ATAN); queries: px_cur 0 in every case, depth 1.1e-12 relative (E, ATAN,
align_1d); seeds: mu 1.1e-7 relative (E, ATAN), sigma2 1.6e-3 of sigma2 on one seed of L10 / radtan (inside the
rule's 4 eps32 (sigma2 + mu^2)) and below 8e-6 elsewhere, a / b 5.5e-6 (L10, radtan), px_cur 0 with sub-pixel refinement and
1.1e-13 px without (E, ATAN: world2cam of uv_best); the resident entry bit for bit the flat one on all three cameras.  The
1e-9 rule on px_cur needed no change on lines of up to 1000 additions."""
import numpy as np
import pytest

import track_edge_cases as cases
import tracking_cases as tc
import tracking_device as td
from helpers import CAMERA_KINDS

pytestmark = pytest.mark.gpu

NAMES = tuple(n for g in cases.COVERAGE for n in cases.COVERAGE[g][0])
GROUP_OF = {n: g for g in cases.COVERAGE for n in cases.COVERAGE[g][0]}


def _case(name, cam_kind):
    c = cases.case(name, cam_kind)
    cases.assert_coverage(GROUP_OF[name], cam_kind)   # (prints the class counts; on the checker and classifier alone)
    return c


@pytest.mark.parametrize("cam_kind", CAMERA_KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_find_match_direct(gpu_device, checker, name, cam_kind):
    c = _case(name, cam_kind)
    worst = tc.verify_matcher(c, *td.find_match_direct(c), which=checker)
    print(f"{name} {cam_kind} [{checker}]: max |dA_cur_ref| {worst:.2e}")


@pytest.mark.parametrize("cam_kind", CAMERA_KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_find_epipolar_match_direct(gpu_device, checker, name, cam_kind):
    c = _case(name, cam_kind)
    for align_1d, cap in [(0, 1000), (1, 1000)] + ([(0, c.cap)] if c.cap else []):
        wpx, wd = tc.verify_epipolar(c, align_1d, cap, *td.find_epipolar(c, c.epi, align_1d, cap), which=checker)
        print(f"{name} {cam_kind} [{checker}] align_1d={align_1d} cap={cap}: max |dpx_cur| {wpx:.2e}, max relative depth difference {wd:.2e}")


@pytest.mark.parametrize("cam_kind", CAMERA_KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_update_seeds(gpu_device, checker, name, cam_kind):
    c = _case(name, cam_kind)
    for align_1d, subpix, cap in [(0, 1, 1000)] + ([(0, 0, 1000), (0, 1, c.cap)] if c.cap else []):
        w = tc.verify_seeds(c, align_1d, subpix, cap, *td.update_seeds(c, align_1d, subpix, cap), which=checker, device=True)
        print(f"{name} {cam_kind} [{checker}] align_1d={align_1d} subpix={subpix} cap={cap}: max deviations {tc.format_deviations(w)}")


@pytest.mark.parametrize("cam_kind", CAMERA_KINDS)
def test_long_lines_on_the_resident_store(gpu_device, oracle, cam_kind):
    """Case E through svo_hip_update_seeds_resident: the bits of the flat entry (tracking_cases.verify_resident) -- statuses,
    points, px_cur, the state in the store and in the dense read-back; slots nobody named untouched."""
    c = _case("E", cam_kind)
    P = c.P
    st0, a, b, mu, s2, xyz0, px0 = td.update_seeds(c, 0, 1, 1000)
    slots = np.random.default_rng(5).permutation(3 * P)[:P].astype(np.int32)
    resident = td.update_seeds_resident(c, slots, (np.arange(P // 2), np.arange(P // 2, P)))
    touched, conv = tc.verify_resident(slots, 3 * P, (st0, xyz0, px0, dict(a=a, b=b, mu=mu, sigma2=s2)), resident)
    print(f"E {cam_kind} resident: {touched} seeds updated, {conv} converged, identical to the flat entry")
