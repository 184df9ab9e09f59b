"""The bootstrap's tracker without a GPU: svo_hip_klt_track and svo_hip_klt_summarize of the host-emulated build
(tests/emu_build.py: klt_track.hip compiled for the CPU through tests/host/hip_emu.h, one fiber per lane, the wave's
exchanges as rendezvous) against the f64 checker (tests/klt_checker.py) on a 376 x 240 camera, 5 levels, 48 corners, frame 0
tracked into the following frames with the carried flow.

At least 99 % of the points of every pair agree with the checker in status and, where tracked, in px_cur within 5e-3 px and
in error within 1e-2 grey levels.  The position bound is derived, not tuned: device (f32) and checker (f64) can disagree
about one stop decision (|delta| <= 1e-3 px, or the half-step rule), which moves the point by about one last step; 5 x
that.  Measured on these scenes (seeds 12345 and 777, max_step 0.03, three pairs each): no status differs, no exception
is used, largest position difference 4.6e-4 px (one point of seed 777's first pair; 3e-5 px on the other five pairs),
largest error difference 3.2e-4 grey levels.
Run once under scripts/emu_sanitize.sh address as well."""
import ctypes as C

import numpy as np
import pytest

import klt_checker
import klt_scenes
from klt_edge_cases import compare_with_checker, PX_TOL, ERR_TOL
from helpers import camera_models, CAMERA_KINDS
from host_buffers import ptr
from rpg_svo_amd import capi


@pytest.fixture(scope="module")
def emu():
    from emu_build import build_emulated
    return build_emulated(())


def default_params(emu):
    p = capi.KltParams()
    assert emu.svo_hip_klt_params_default(C.byref(p)) == 0
    return p


def build_store(emu, images, n_levels=5):
    n, h, w = images.shape
    layout = capi.pyr_layout(w, h, n_levels)      # (host-only helpers of the library proper, as in the other emulated tests)
    store = np.zeros(capi.pyr_store_bytes(layout, n), np.uint8)
    images = np.ascontiguousarray(images)
    assert emu.svo_hip_pyramid_build_tiled(C.byref(layout), ptr(store), 0, n, ptr(images), C.c_longlong(h * w), w, capi.HALFSAMPLE_AUTO, 0, None) == 0
    return layout, store


def klt_track(emu, layout, store, ref_slot, cur_slot, px_ref, px_cur, status, error=None, params=None):
    """px_ref [n_pairs, n_pts, 2] f32; px_cur, status in/out (copies are returned)"""
    n_pairs, n_pts = px_ref.shape[:2]
    px_ref = np.ascontiguousarray(px_ref, np.float32)
    px_cur = np.ascontiguousarray(px_cur, np.float32).copy()
    status = np.ascontiguousarray(status, np.uint8).copy()
    error = np.zeros((n_pairs, n_pts), np.float32) if error is None else error.copy()
    rs, cs = np.asarray(ref_slot, np.int32), np.asarray(cur_slot, np.int32)
    params = params or default_params(emu)
    rc = emu.svo_hip_klt_track(C.byref(layout), ptr(store), n_pairs, ptr(rs), ptr(cs), n_pts, ptr(px_ref), ptr(px_cur), ptr(status), ptr(error),
                               C.byref(params), None)
    assert rc == 0, rc
    return px_cur, status, error


@pytest.mark.parametrize("seed", [12345, 777])
def test_emulated_klt_against_checker(emu, oracle, seed):
    cam = klt_scenes.small_camera()
    s = klt_scenes.make_scene(seed, 0.03, 4, cam=cam, n_corners=48)
    pyrs = [oracle.create_img_pyramid(im, 5) for im in s.images]
    chain = klt_scenes.checker_chain(pyrs, s.px_ref)
    layout, store = build_store(emu, s.images)
    n_pairs = len(chain)
    px_ref = np.broadcast_to(s.px_ref, (n_pairs, 48, 2))
    px_in = np.stack([c["px_in"] for c in chain])
    st_in = np.stack([c["st_in"] for c in chain])
    px, st, err = klt_track(emu, layout, store, [0] * n_pairs, list(range(1, n_pairs + 1)), px_ref, px_in, st_in)
    assert st.sum() >= 0.7 * st.size   # the scene is tracked at this size as well
    for k in range(n_pairs):
        compare_with_checker(f"seed {seed} pair {k}", px[k], st[k], err[k], chain[k])
        # against the renderer: the conditions of tests/test_klt_checker.py hold for the device's result as well
        ok, ttext = klt_scenes.truth_violations(cam, s.truth[k + 1], px[k].astype(np.float64), st[k])
        print(ttext)
        assert ok, ttext
    # a second call gives the same bits (fixed summation order)
    px2, st2, err2 = klt_track(emu, layout, store, [0] * n_pairs, list(range(1, n_pairs + 1)), px_ref, px_in, st_in)
    assert np.array_equal(px.view(np.uint32), px2.view(np.uint32)) and np.array_equal(st, st2) and np.array_equal(err.view(np.uint32), err2.view(np.uint32))


@pytest.fixture(scope="module")
def small_scene(emu):
    cam = klt_scenes.small_camera()
    s = klt_scenes.make_scene(12345, 0.03, 2, cam=cam, n_corners=48)
    s.layout, s.store = build_store(emu, s.images)
    return s


def test_input_status_zero_leaves_the_outputs_untouched(emu, small_scene):
    s = small_scene
    n = 16
    px_ref = s.px_ref[None, :n]
    st_in = np.ones((1, n), np.uint8)
    st_in[0, ::3] = 0
    px_in = px_ref.copy()
    px_in[0, ::3] = np.float32(-777.25)                   # poison
    err_in = np.full((1, n), np.float32(123.5))
    px, st, err = klt_track(emu, s.layout, s.store, [0], [1], px_ref, px_in, st_in, error=err_in)
    lost = st_in[0] == 0
    assert (px[0, lost] == np.float32(-777.25)).all() and (st[0, lost] == 0).all() and (err[0, lost] == np.float32(123.5)).all()
    assert (st[0, ~lost] == 1).all() and (err[0, ~lost] != np.float32(123.5)).all()
    # and the other points do not depend on their neighbours in the batch
    px1, st1, err1 = klt_track(emu, s.layout, s.store, [0], [1], px_ref[:, 1:2], px_ref[:, 1:2], np.ones((1, 1), np.uint8))
    assert np.array_equal(px1[0, 0].view(np.uint32), px[0, 1].view(np.uint32)) and err1[0, 0] == err[0, 1]


def test_flat_image_loses_every_point(emu):
    flat = np.full((2, 240, 376), 127, np.uint8)
    layout, store = build_store(emu, flat)
    px_ref = np.array([[[60.0, 60.0], [188.0, 120.0], [300.5, 200.25], [20.0, 15.0]]], np.float32)
    px, st, err = klt_track(emu, layout, store, [0], [1], px_ref, px_ref, np.ones((1, 4), np.uint8), error=np.full((1, 4), np.float32(9.0)))
    assert (st == 0).all() and (err == 0.0).all()          # min_eig below the threshold at level 0


def test_initial_flow_is_honoured(emu, small_scene):
    s = small_scene
    n = 8
    px_ref = s.px_ref[None, :n]
    ones = np.ones((1, n), np.uint8)
    answer, st, _ = klt_track(emu, s.layout, s.store, [0], [1], px_ref, px_ref, ones)
    assert (st == 1).all()
    from_answer, st_a, _ = klt_track(emu, s.layout, s.store, [0], [1], px_ref, answer, ones)
    off = answer + np.array([2.0, -2.236], np.float32)     # 3 px away
    from_off, st_o, _ = klt_track(emu, s.layout, s.store, [0], [1], px_ref, off, ones)
    assert (st_a == 1).all() and (st_o == 1).all()
    d = np.abs(from_answer.astype(np.float64) - from_off).max()
    print(f"started at the answer vs 3 px off: max difference {d:.2e} px")
    assert d <= PX_TOL
    # a start at the answer stays there: the initial flow is used, not replaced by px_ref
    assert np.abs(from_answer.astype(np.float64) - answer).max() <= PX_TOL
    assert np.abs(answer - px_ref).max() > 1.0
    # with no iteration allowed the flow comes back as it went in (division and multiplication by 2^L are exact)
    frozen = default_params(emu)
    frozen.max_iter = 0
    kept, st_k, err_k = klt_track(emu, s.layout, s.store, [0], [1], px_ref, off, ones, params=frozen)
    assert np.array_equal(kept.view(np.uint32), off.view(np.uint32)) and (st_k == 1).all() and (err_k > 0).all()


def test_no_points_and_error_codes(emu, small_scene):
    s = small_scene
    L, store = s.layout, s.store
    p = default_params(emu)
    assert (p.win_size, p.max_level, p.max_iter) == (30, 4, 30) and p.eps == np.float32(1e-3) and p.min_eig_threshold == np.float32(1e-4)
    assert emu.svo_hip_klt_params_default(None) == -1
    rs, cs = np.zeros(1, np.int32), np.ones(1, np.int32)
    px = s.px_ref[None, :4].copy()
    st, err = np.ones((1, 4), np.uint8), np.zeros((1, 4), np.float32)

    def call(layout=L, store_=store, n_pairs=1, n_pts=4, px_ref=px, px_cur=px, status=st, error=err, params=p, rs_=rs, cs_=cs):
        return emu.svo_hip_klt_track(None if layout is None else C.byref(layout), ptr(store_), n_pairs, ptr(rs_), ptr(cs_), n_pts, ptr(px_ref),
                                     ptr(px_cur), ptr(status), ptr(error), None if params is None else C.byref(params), None)

    assert call(n_pts=0) == 0 and call(n_pairs=0) == 0      # successful no-ops
    assert call(n_pts=0, px_ref=None, px_cur=None, status=None, error=None) == 0
    assert call(n_pts=-1) == -1 and call(n_pairs=-1) == -1
    assert call(layout=None) == -1 and call(params=None) == -1
    for missing in ("store_", "px_ref", "px_cur", "status", "error", "rs_", "cs_"):
        assert call(**{missing: None}) == -1, missing
    rowmajor = capi.PyrLayout.from_buffer_copy(L)
    rowmajor.tile = capi.PYR_ROWMAJOR
    assert call(layout=rowmajor) == -1
    deep = capi.KltParams.from_buffer_copy(p)
    deep.max_level = L.n_levels
    assert call(params=deep) == -1
    win = capi.KltParams.from_buffer_copy(p)
    win.win_size = 21
    assert call(params=win) == -2
    assert call(n_pts=1025) == -2
    cam = capi.camera(s.cam)
    f, d, n, m = np.zeros((1, 4, 3)), np.zeros((1, 4)), np.zeros(1, np.int32), np.zeros(1)
    pxc = px.copy()
    assert emu.svo_hip_klt_summarize(C.byref(cam), 1, 4, ptr(px), ptr(pxc), ptr(st), ptr(f), ptr(d), ptr(n), ptr(m), None) == 0
    assert emu.svo_hip_klt_summarize(None, 1, 4, ptr(px), ptr(pxc), ptr(st), ptr(f), ptr(d), ptr(n), ptr(m), None) == -1
    assert emu.svo_hip_klt_summarize(C.byref(cam), 1, 4, ptr(px), ptr(pxc), ptr(st), None, ptr(d), ptr(n), ptr(m), None) == -1
    assert emu.svo_hip_klt_summarize(C.byref(cam), 1, 1025, ptr(px), ptr(pxc), ptr(st), ptr(f), ptr(d), ptr(n), ptr(m), None) == -2
    assert emu.svo_hip_klt_summarize(C.byref(cam), 0, 4, None, None, None, None, None, None, None, None) == 0
    bad = capi.camera(s.cam)
    bad.model = 7
    assert emu.svo_hip_klt_summarize(C.byref(bad), 1, 4, ptr(px), ptr(pxc), ptr(st), ptr(f), ptr(d), ptr(n), ptr(m), None) == -1


@pytest.mark.parametrize("kind", CAMERA_KINDS)
def test_summary_step(emu, kind):
    cam = camera_models()[kind]
    ccam = capi.camera(cam)
    rng = np.random.default_rng(5)
    n_pairs, n_pts = 4, 301
    px_ref = rng.uniform(30, 440, (n_pairs, n_pts, 2)).astype(np.float32)
    px_cur = (px_ref + rng.normal(0, 30, px_ref.shape)).astype(np.float32)
    px_cur[1, 10:40] = px_cur[1, 9]          # ties in the disparities
    px_ref[1, 10:40] = px_ref[1, 9]
    st = (rng.uniform(size=(n_pairs, n_pts)) < 0.8).astype(np.uint8)
    st[2] = 0                                 # a pair with nothing tracked
    st[3] = 0
    st[3, 17] = 1                             # and one with a single point
    f = np.full((n_pairs, n_pts, 3), np.nan)
    d = np.full((n_pairs, n_pts), np.nan)
    n = np.full(n_pairs, -1, np.int32)
    med = np.full(n_pairs, np.nan)
    assert emu.svo_hip_klt_summarize(C.byref(ccam), n_pairs, n_pts, ptr(px_ref), ptr(px_cur), ptr(st), ptr(f), ptr(d), ptr(n), ptr(med), None) == 0
    # bearings: the bits of svo_hip_cam2world on the same pixels
    f_ref = np.zeros((n_pairs * n_pts, 3))
    px64 = np.ascontiguousarray(px_cur.reshape(-1, 2).astype(np.float64))
    assert emu.svo_hip_cam2world(C.byref(ccam), n_pairs * n_pts, ptr(px64), ptr(f_ref), None) == 0
    on = st.reshape(-1) != 0
    assert np.array_equal(f.reshape(-1, 3)[on].view(np.uint64), f_ref[on].view(np.uint64))
    assert (f.reshape(-1, 3)[~on] == 0).all() and (d.reshape(-1)[~on] == 0).all()
    assert np.allclose(np.linalg.norm(f.reshape(-1, 3)[on], axis=1), 1.0, atol=1e-12)
    for k in range(n_pairs):
        dk, nk, mk = klt_checker.summarize(px_ref[k], px_cur[k], st[k])
        assert n[k] == nk
        assert np.array_equal(d[k].view(np.uint64), dk.view(np.uint64))
        assert med[k:k + 1].view(np.uint64)[0] == np.array([mk]).view(np.uint64)[0], (k, med[k], mk)
        if nk:
            assert mk == sorted(dk[st[k] != 0])[nk // 2]
    assert n[2] == 0 and med[2] == 0.0 and n[3] == 1
