"""Rows a8-a10 without a GPU: svo_hip_find_match_direct of the host-emulated library (tests/emu_build.py: matcher.hip and
feature_align.hip compiled for the CPU through tests/host/hip_emu.h) -- match_prepare, warp_kernel with its LDS regions
and same-wave hand-overs, align_kernel -- against the oracle's Matcher::findMatchDirect on the scene of the GPU test, with
the same requirements: verdicts, chosen observations, search levels and the 10 x 10 patches identical, refined pixels
identical in every bit, A to 1e-12.  Also with the queued opt-in builds, whose results must not differ from the default's."""
import numpy as np
import pytest

import tracking_cases as tc
import tracking_emulated as te


@pytest.fixture(scope="module", params=[0], ids=["default"])
def emu(request):
    from emu_build import build_emulated
    from emu_build import BUILDS
    return build_emulated(BUILDS[request.param])


@pytest.fixture(scope="module", params=["pinhole", "atan"])
def case(request):
    return tc.committed(request.param)


def test_emulated_find_match_direct(emu, oracle, case):
    tc.verify_matcher(case, *te.find_match_direct(emu, case))
    n_ok, n_edge = tc.matcher_coverage(case)
    assert n_ok > 200 and n_edge > 20


# ---- row a12: svo_hip_update_seeds (seed_prepare -> warp -> epipolar scan -> alignment -> seed_finish) -----------------


@pytest.fixture(scope="module", params=[0, 1], ids=["default", "lane_kernel_with_finish"])
def emu_seeds(request):
    from emu_build import build_emulated
    from emu_build import BUILDS
    return build_emulated(BUILDS[request.param])


@pytest.mark.parametrize("align_1d,subpix", [(0, 1), (1, 1), (0, 0)])
def test_emulated_update_seeds(emu_seeds, oracle, case, align_1d, subpix):
    """DepthFilter::updateSeeds as the five kernels of svo_hip_update_seeds run it, on the CPU, with the requirements of the
    GPU test (tracking_cases.verify_seeds; sigma2 by the emulation's rule), in list order and keyframe by keyframe
    (tracking_cases.seed_order): the same bits either way.  subpix=0: Matcher::Options::subpix_refinement == false -- a scan
    match is triangulated straight from uv_best (matcher.cpp:316-318) instead of being refined by align1D/align2D."""
    first = te.update_seeds(emu_seeds, case, align_1d, subpix, 1000)
    order = tc.seed_order(case)
    tc.verify_seed_order(order, first, te.update_seeds(emu_seeds, case, align_1d, subpix, 1000, order))
    tc.verify_seeds(case, align_1d, subpix, 1000, *first)
    tc.seed_coverage(case, "orc", align_1d, subpix)


def test_emulated_update_seeds_on_the_resident_store(emu_seeds, case):
    """Row N2, seeds, on the CPU (tracking_cases.verify_resident): the seeds scattered over a resident store
    (svo_hip_seed_store_patch, two instalments) and updated in list order through svo_hip_update_seeds_resident give the bits
    svo_hip_update_seeds gives on the flattened list, and leave every other slot alone; svo_hip_update_seeds_resident_pose on a
    second store patched with the same records in one instalment: the same bits."""
    S = case.P
    st0, a, b, mu, s2, xyz0, px0, *_ = te.update_seeds(emu_seeds, case, 0, 1, 1000)
    slots = tc.resident_slots(case)
    resident = te.update_seeds_resident(emu_seeds, case, slots, (np.arange(S // 2), np.arange(S // 2, S)))
    by_pose = te.update_seeds_resident(emu_seeds, case, slots, (np.arange(S),), by_pose=True)
    touched, conv = tc.verify_resident(slots, 3 * S, (st0, xyz0, px0, dict(a=a, b=b, mu=mu, sigma2=s2)), resident, by_pose)
    assert conv > 2 and touched > 100
