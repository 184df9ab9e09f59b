"""svo_hip_find_match_direct, svo_hip_find_epipolar_match_direct and svo_hip_update_seeds* of the host-emulated build
(tests/emu_build.py) on the cases of tests/track_edge_cases.py: feature and search levels 0 to 4 on both sides of each
other (L), the gather path of the affine warp (Z), features and projections at and beyond the borders with the clamped
source box, warp_sample<true> and the all-zero patch (B), epipolar lines from under two pixels to beyond the cap of 1000
steps through every bucket of the scan's counting sort, with the box per half group on the ATAN camera (E) -- against
the checker by the rules of tests/test_track_emulated.py and tests/test_entries_emulated.py, unchanged.  The coverage
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
import ctypes as C

import numpy as np
import pytest

import track_edge_cases as cases
from host_buffers import ptr
from oracle import pytrack
from rpg_svo_amd import capi

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


def _store(emu, images):
    imgs = np.ascontiguousarray(images)
    n, h, w = imgs.shape
    layout = capi.pyr_layout(w, h, cases.N_LEVELS)
    buf = np.zeros(capi.pyr_store_bytes(layout, n), np.uint8)
    assert emu.svo_hip_pyramid_build_tiled(C.byref(layout), ptr(buf), 0, n, ptr(imgs), C.c_longlong(h * w), w, capi.HALFSAMPLE_AUTO, 0, None) == 0
    return layout, buf


def _features(cols):
    return capi.Features(*[cols[k].ctypes.data for k in ("frame", "level", "type", "px", "f", "grad")])


def _workspace(emu, n):
    emu.svo_hip_match_workspace_bytes.restype = C.c_size_t
    return np.full(emu.svo_hip_match_workspace_bytes(n) + 256, 0xFF, np.uint8)   # (poisoned)


def _frames(T):
    slots = np.arange(T.shape[0], dtype=np.int32)
    fr = capi.Frames(T.shape[0], 0, slots.ctypes.data, T.ctypes.data)
    fr._keep = (slots, T)
    return fr


@pytest.mark.parametrize("cam_kind", CAMS)
@pytest.mark.parametrize("group", GROUPS)
def test_coverage(oracle, group, cam_kind):
    """the classes a group of cases exists for are reached, by the checker's and the classifier's account"""
    cases.assert_coverage(group, cam_kind)


@pytest.mark.parametrize("cam_kind", CAMS)
@pytest.mark.parametrize("name", NAMES)
def test_find_match_direct(emu, oracle, name, cam_kind):
    c = cases.case(name, cam_kind)
    s, P = c.scene, c.P
    layout, store = _store(emu, s.images)
    frames, obs, cam = _frames(c.T_match), _features(c.obs_cols), capi.camera(s.cam)
    cur, pos, px = np.full(P, s.cur, np.int32), np.ascontiguousarray(s.pt_pos), np.ascontiguousarray(s.px_init).copy()
    ok, ref_obs, sl = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int32)
    A, patches = np.zeros((P, 4)), np.zeros((P, 100), np.uint8)
    ws = _workspace(emu, P)
    rc = emu.svo_hip_find_match_direct(C.byref(layout), ptr(store), C.byref(cam), C.byref(frames), P, ptr(cur), ptr(pos), ptr(c.obs_ptr), C.byref(obs),
                                       cases.N_LEVELS, 10, ptr(px), ptr(ok), ptr(ref_obs), ptr(sl), ptr(A), ptr(patches), ptr(ws), C.c_size_t(ws.size), None)
    assert rc == 0, rc
    worst = cases.verify_matcher(c, ok, px, ref_obs, sl, A, patches)
    print(f"{name} {cam_kind}: max |dA_cur_ref| {worst:.2e}")


def _epipolar(emu, c, layout, store, align_1d, cap):
    s, P = c.scene, c.P
    frames, ftr, cam = _frames(np.ascontiguousarray(s.T_f_w)), _features(c.ftr_cols), capi.camera(s.cam)
    cur = np.full(P, s.cur, np.int32)
    de, dmin, dmax = (np.ascontiguousarray(x) for x in (c.d_est, c.d_min, c.d_max))
    o_ = capi.DepthFilterOptions(0, 0, 0.0, int(align_1d), 10, cap, 1, 1, cases.N_LEVELS, 0.7)
    ok, depth, px, lvl = np.zeros(P, np.int32), np.zeros(P), np.zeros((P, 2)), np.zeros(P, np.int32)
    ws = _workspace(emu, P)
    rc = emu.svo_hip_find_epipolar_match_direct(C.byref(layout), ptr(store), C.byref(cam), C.byref(frames), P, ptr(cur), C.byref(ftr), ptr(de),
                                                ptr(dmin), ptr(dmax), C.byref(o_), ptr(ok), ptr(depth), ptr(px), ptr(lvl), ptr(ws), C.c_size_t(ws.size), None)
    assert rc == 0, rc
    return ok, depth, px, lvl


@pytest.mark.parametrize("cam_kind", CAMS)
@pytest.mark.parametrize("name", NAMES)
def test_find_epipolar_match_direct(emu, oracle, name, cam_kind):
    c = cases.case(name, cam_kind)
    layout, store = _store(emu, c.scene.images)
    runs = [(0, 1000), (1, 1000)] + ([(0, c.cap)] if c.cap else [])
    for align_1d, cap in runs:
        wpx, wd = cases.verify_epipolar(c, align_1d, cap, *_epipolar(emu, c, layout, store, align_1d, cap))
        print(f"{name} {cam_kind} align_1d={align_1d} cap={cap}: max |dpx_cur| {wpx:.2e}, max relative depth difference {wd:.2e}")
    if c.cap:   # the smaller cap really fired
        free, capped = c.epi_ref("orc", 0, 1000), c.epi_ref("orc", 0, c.cap)
        assert sum(1 for a, b in zip(free, capped) if a[0] and not b[0]) >= cases.MIN_REJECTED


def _update_seeds(emu, c, layout, store, align_1d, subpix, cap):
    s, P = c.scene, c.P
    frames, ftr, cam = _frames(np.ascontiguousarray(s.T_f_w)), _features(c.ftr_cols), capi.camera(s.cam)
    st = {k: v.copy() for k, v in c.seed_cols.items()}
    sd = capi.Seeds(*[st[k].ctypes.data for k in ("a", "b", "mu", "z_range", "sigma2", "batch_id")])
    dopt = capi.DepthFilterOptions(3, 5, 200.0, int(align_1d), 10, cap, int(subpix), 1, cases.N_LEVELS, 0.7)
    cur = np.full(P, s.cur, np.int32)
    status, xyz, px = np.zeros(P, np.int32), np.zeros((P, 3)), np.zeros((P, 2))
    ws = _workspace(emu, P)
    rc = emu.svo_hip_update_seeds(C.byref(layout), ptr(store), C.byref(cam), C.byref(frames), P, ptr(cur), C.byref(ftr), C.byref(sd), C.byref(dopt),
                                  ptr(status), ptr(xyz), ptr(px), ptr(ws), C.c_size_t(ws.size), None)
    assert rc == 0, rc
    return status, st["a"], st["b"], st["mu"], st["sigma2"], xyz, px


@pytest.mark.parametrize("cam_kind", CAMS)
@pytest.mark.parametrize("name", NAMES)
def test_update_seeds(emu_seeds, oracle, name, cam_kind):
    c = cases.case(name, cam_kind)
    layout, store = _store(emu_seeds, c.scene.images)
    runs = [(0, 1, 1000)] + ([(0, 0, 1000), (0, 1, c.cap)] if c.cap else [])
    for align_1d, subpix, cap in runs:
        w = cases.verify_seeds(c, align_1d, subpix, cap, *_update_seeds(emu_seeds, c, layout, store, align_1d, subpix, cap))
        print(f"{name} {cam_kind} align_1d={align_1d} subpix={subpix} cap={cap}: max deviations " + ", ".join(f"{k} {v:.2e}" for k, v in w.items()))
    if c.cap:
        free, capped = c.seeds_ref("orc", 0, 1, 1000)[1], c.seeds_ref("orc", 0, 1, c.cap)[1]
        assert sum(1 for a, b in zip(free, capped) if a.status in cases.OK_SEED and b.status == pytrack.SEED_NO_MATCH) >= cases.MIN_REJECTED
