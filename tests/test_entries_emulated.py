"""The remaining C-ABI entry points of the tracking kernels without a GPU (host-emulated library, tests/emu_build.py), each with
the requirements of its GPU test in tests/test_tracking_gpu.py: svo_hip_align_batch / _counted / _phased (the phased form --
three launches, survivors compacted through atomically filled queues, parked loop state -- starts at 2048 trials in the
emulated build), svo_hip_find_epipolar_match_direct, svo_hip_update_seed_batch, svo_hip_compute_tau_batch,
svo_hip_select_matches, svo_hip_compose_poses, svo_hip_cam2world.  Cases and rules: tests/tracking_cases.py; the calls:
tests/tracking_emulated.py.  The draws of this file do not move with SVO_TEST_FUZZ."""
import ctypes as C

import numpy as np
import pytest

import tracking_cases as tc
import tracking_emulated as te
from helpers import camera_models
from host_buffers import ptr
from oracle import pytrack
from rpg_svo_amd import capi, se3, synth


@pytest.fixture(scope="module", params=[0], ids=["default"])
def emu(request):
    from emu_build import BUILDS, build_emulated
    return build_emulated(BUILDS[request.param])


@pytest.fixture(scope="module")
def emu_default():
    """(the default build only: tests of kernels no queued flag touches)"""
    from emu_build import build_emulated
    return build_emulated(())


@pytest.fixture(scope="module")
def scene():
    return synth.make_track_scene(n_kf=4, n_feat=100, cam=camera_models()["pinhole"])


@pytest.fixture(scope="module")
def case(scene):
    return tc.of_scene(scene, "entries", rng=np.random.default_rng)


def _store(emu, images):
    return te.pyramid_store(emu, np.ascontiguousarray(images))


def test_emulated_align_batch_and_its_phased_form(emu, oracle, case):
    orc, pyrs, _, _ = case.checker("orc")
    layout, store, _ = te.store_and_frames(emu, case, case.T_f_w)
    tr = tc.align_trials(pyrs, np.random.default_rng(3), 4096, 4.0)
    M, n_iter = 4096, 10
    single = te.align_batch(emu, layout, store, tr, n_iter)
    ev_c = np.zeros(M, np.int32)
    counted = te.align_batch(emu, layout, store, tr, n_iter, "_counted", (ptr(ev_c),))
    emu.svo_hip_align_workspace_bytes.restype = C.c_size_t
    need = emu.svo_hip_align_workspace_bytes(M)
    assert need > 0                                                     # (the emulated build's threshold: the phased path)
    raw, ev_p = np.full(need + 512, 0xFF, np.uint8), np.zeros(M, np.int32)
    ws = raw[(-raw.ctypes.data) % 256:][:need + 256]                     # (the entry wants 256-byte alignment, like hipMalloc's)
    phased = te.align_batch(emu, layout, store, tr, n_iter, "_phased", (ptr(ev_p), ptr(ws), C.c_size_t(ws.size)))
    tc.same_alignment(counted, single)
    tc.same_alignment(phased + (ev_p,), single + (ev_c,))
    assert (ev_c > 6).sum() > 20 and (ev_c <= 3).sum() > 100, np.bincount(ev_c)   # all three launches had work
    px_a, ok_a, h_a = single
    assert tc.check_alignment(orc, pyrs, tr, n_iter, ok_a, px_a, h_a, every=4) > M // 16   # the single launch against the reference's functions


@pytest.mark.parametrize("n_iter", [0, 1, 3, 10])
def test_emulated_wave_alignment_iteration_caps_and_borders(emu, oracle, scene, n_iter):
    """The wave-per-trial kernel (csrc/align_wave.h: batches of up to 8192 trials) against the reference's align2D / align1D
    at iteration caps 0 / 1 / 3 / 10 (Matcher::Options::align_max_iter), with starts on the rim of the valid region (the
    first bounds test fails / the position leaves after a step), flat templates (singular H: NaN updates) and templates from
    a different place (chi2 rises: align1D's early exit): verdict, refined pixel, h_inv and evaluation count per trial."""
    orc = pytrack.Track("orc")
    imgs = scene.images.cpu().numpy()
    pyrs = [orc.create_img_pyramid(im, 5) for im in imgs]
    layout, store = _store(emu, imgs)
    rng = np.random.default_rng(100 + n_iter)
    M = 192
    slot = rng.integers(0, imgs.shape[0], size=M).astype(np.int32)
    level = rng.integers(0, 4, size=M).astype(np.int32)
    pwb, px0 = np.zeros((M, 100), np.uint8), np.zeros((M, 2))
    dirs = rng.normal(size=(M, 2)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    use_1d = (np.arange(M) % 2).astype(np.uint8)
    for t in range(M):
        img = pyrs[slot[t]][level[t]]
        h, w = img.shape
        u, v = rng.integers(8, w - 8), rng.integers(8, h - 8)
        kind = t % 6
        src = pyrs[(slot[t] + 1) % imgs.shape[0]][level[t]]
        pwb[t] = src[v - 5:v + 5, u - 5:u + 5].ravel()
        px0[t] = [u + rng.uniform(-3.0, 3.0), v + rng.uniform(-3.0, 3.0)]
        if kind == 1:
            px0[t] = [4.0 + rng.uniform(0, 0.9), v]                     # on the rim: inside now, one step from leaving
        elif kind == 2:
            px0[t] = [w - 4.0 + rng.uniform(0, 0.5), v]                 # the first bounds test fails: no evaluation
        elif kind == 3:
            pwb[t] = 128                                                # flat template: singular H
        elif kind == 4:
            uu, vv = rng.integers(8, w - 8), rng.integers(8, h - 8)     # a template from somewhere else
            pwb[t] = img[vv - 5:vv + 5, uu - 5:uu + 5].ravel()
    px, ok, h_inv, ev = px0.copy(), np.zeros(M, np.int32), np.zeros(M), np.full(M, -1, np.int32)
    rc = emu.svo_hip_align_batch_counted(C.byref(layout), ptr(store), M, ptr(slot), ptr(level), ptr(pwb), ptr(dirs), ptr(use_1d), n_iter, ptr(px),
                                         ptr(ok), ptr(h_inv), ptr(ev), None)
    assert rc == 0
    assert ev.min() >= 0 and ev.max() <= n_iter and (n_iter == 0 or (ev == 0).sum() >= M // 8)
    for t in range(M):
        img = pyrs[slot[t]][level[t]]
        patch = pwb[t].reshape(10, 10)[1:9, 1:9].ravel()
        if use_1d[t]:
            o, p, hi = orc.align1d(img, dirs[t], pwb[t], patch, n_iter, px0[t])
            assert hi == h_inv[t] or (np.isnan(hi) and np.isnan(h_inv[t])) or (np.isinf(hi) and np.isinf(h_inv[t])), (t, hi, h_inv[t])
        else:
            o, p = orc.align2d(img, pwb[t], patch, n_iter, px0[t])
        assert bool(ok[t]) == o, (t, n_iter)
        assert np.array_equal(p, px[t], equal_nan=True), (t, n_iter, p, px[t])


def test_emulated_find_epipolar_match_direct(emu, oracle, case):
    for align_1d in (0, 1):
        tc.verify_epipolar(case, align_1d, 1000, *te.find_epipolar(emu, case, case.epi, align_1d, 1000))
        assert sum(r[0] for r in case.epi_ref("orc", align_1d)) > case.epi.n // 3


def test_emulated_update_seed_and_compute_tau_batches(emu, oracle):
    orc = pytrack.Track("orc")
    rng = np.random.default_rng(6)
    seeds, cols, x, tau2 = tc.seed_batch(orc, rng, 3000)
    # host-compiled without contraction, libm's exp on both sides: the reference's bits in all but a few seeds
    tc.check_seed_batch(orc, seeds, x, tau2, te.update_seed_batch(emu, cols, x, tau2), min_identical=0.97)
    # computeTau for S independent measurements
    n = 500
    t_rc = rng.normal(size=(n, 3)) * 0.3
    f = rng.normal(size=(n, 3)) * 0.3 + np.array([0, 0, 1.0])
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    z = rng.uniform(0.5, 10.0, size=n)
    ang = np.arctan(1.0 / (2.0 * 315.5)) * 2.0
    tau = np.zeros(n)
    t_rc, f = np.ascontiguousarray(t_rc), np.ascontiguousarray(f)
    assert emu.svo_hip_compute_tau_batch(n, ptr(t_rc), ptr(f), ptr(z), C.c_double(ang), ptr(tau), None) == 0
    for i in range(n):
        T = np.concatenate([np.eye(3).ravel(), t_rc[i]])
        want_tau = orc.compute_tau(T, f[i], z[i], ang)
        assert np.isnan(tau[i]) == np.isnan(want_tau)
        if not np.isnan(want_tau):
            assert abs(tau[i] - want_tau) <= 1e-9 * abs(want_tau), (i, tau[i], want_tau)   # (bit-equal in the default build)


@pytest.mark.parametrize("kind", ["pinhole", "atan"])
def test_emulated_select_matches_compose_poses_cam2world(emu_default, oracle, kind):
    emu = emu_default
    cam = camera_models()[kind]
    cs = capi.camera(cam)
    rng = np.random.default_rng(77)
    for M, max_fts in tc.SELECT_SHAPES_EMULATED:
        trials = tc.select_trials(cam, rng, M)
        tc.check_select_matches(cam, trials, max_fts, *te.select_matches(emu, cam, *trials, max_fts))
    # glue: SE(3) products (optionally scattered) and bearings
    n = 300
    A = np.stack([se3.exp(rng.normal(size=6) * 0.3) for _ in range(n)])
    B = np.stack([se3.exp(rng.normal(size=6) * 0.3) for _ in range(n)])
    out = np.zeros((n, 12))
    assert emu.svo_hip_compose_poses(n, ptr(A), ptr(B), ptr(out), None, None) == 0
    assert np.abs(out - se3.mul(A, B)).max() < 1e-14
    idx = rng.permutation(n).astype(np.int32)
    out2 = np.zeros((n, 12))
    assert emu.svo_hip_compose_poses(n, ptr(A), ptr(B), ptr(out2), ptr(idx), None) == 0
    assert np.array_equal(out2[idx], out)
    px = np.ascontiguousarray(np.stack([rng.uniform(0, cam.width, n), rng.uniform(0, cam.height, n)], axis=1))
    fb = np.zeros((n, 3))
    assert emu.svo_hip_cam2world(C.byref(cs), n, ptr(px), ptr(fb), None) == 0
    assert np.abs(fb - synth._bearing(cam, px)).max() < 1e-14


def test_emulated_frame_pose_compose_is_the_hosts_product(emu_default):
    """svo_hip_frame_pose_compose (round 6: the frame's pose formed on the stream behind K1, rpg_svo_amd/host/dropin/
    frame_chain.h) gives, bit for bit, the rotation matrix and translation the host gets from SE3(R, t) * T_ref -- the check
    Reprojector::reprojectMap's drop-in makes before it takes the batch the chain enqueued -- and ranks the overlapping
    keyframes like Map::getCloseKeyframes + the reprojector's sort."""
    emu = emu_default
    rng = np.random.default_rng(5)
    for T, q, t in tc.frame_pose_compose_cases(rng):
        table = np.zeros((3, 12)); copy = np.zeros(12); out = np.zeros(12); sig = np.zeros(1, np.int32)
        assert emu.svo_hip_frame_pose_compose(ptr(T), ptr(q), ptr(t), ptr(table), 1, ptr(copy), ptr(out), None, 0, 0, None, None, 0, None, None,
                                              ptr(sig), 7, None) == 0
        want = tc.host_frame_pose(T, q, t)
        assert np.array_equal(table[1], want) and np.array_equal(copy, want) and np.array_equal(out, want) and sig[0] == 7
        assert not table[0].any() and not table[2].any()
    assert emu.svo_hip_frame_pose_compose(None, ptr(q), ptr(t), ptr(table), 1, None, None, None, 0, 0, None, None, 0, None, None, None, 0,
                                          None) == -1  # SVO_HIP_EINVAL
    # the ranking, on the undistorted pinhole (the distorted models' projection has its own bit-exact tests)
    cam = camera_models()["pinhole"]
    cs = capi.camera(cam)
    for trial in range(40):
        table, key_pos, key_valid = tc.keyframe_rank_case(rng)
        n_tab, n_kf = len(table), len(key_pos)
        T = np.ascontiguousarray(se3.exp(rng.normal(size=6) * 0.05)); q = rng.normal(size=4); q /= np.linalg.norm(q); t = rng.normal(size=3) * 0.2
        for max_n in (3, 10):
            tab = table.copy(); rank = np.full(n_tab, 99, np.int32); rank2 = np.full(n_tab, 99, np.int32)
            assert emu.svo_hip_frame_pose_compose(ptr(T), ptr(q), ptr(t), ptr(tab), n_tab - 2, None, None, C.byref(cs), n_tab, n_kf, ptr(key_pos),
                                                  ptr(key_valid), max_n, ptr(rank), ptr(rank2), None, 0, None) == 0
            want = tc.host_keyframe_ranks(cam, tc.host_frame_pose(T, q, t), tc.composed_quat(T, q), key_pos, key_valid, tab, n_kf, max_n)
            assert np.array_equal(rank, want) and np.array_equal(rank2, want), (trial, rank, want)
            assert (rank[n_kf:] == -1).all() and rank.max() < max_n and rank[7] == -1
            if want[3] >= 0 and want[5] >= 0:
                assert want[5] == want[3] + 1  # equal distances: map order


def test_emulated_indirect_match_batch_is_the_direct_one(emu, scene, case):
    """svo_hip_find_match_direct_indirect / svo_hip_select_matches_indirect (batch size read by the kernels, observation ranges
    instead of CSR offsets: what follows svo_hip_reproject_map on the mirror's path) against the plain entry points on the
    same trials: identical outputs, nothing written beyond the device-side batch size (tests/test_map_mirror_gpu.py)."""
    layout, store, frames = te.store_and_frames(emu, case, case.T_match)
    M, obs_ptr, obs, cam = case.P, case.obs_ptr, te.features(case.obs_cols), capi.camera(scene.cam)
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
    emu.svo_hip_match_workspace_bytes.restype = C.c_size_t
    cap = M + 37
    pad = lambda x: np.ascontiguousarray(np.concatenate([x, np.zeros((cap - M,) + x.shape[1:], x.dtype)]))
    cur, pos = np.full(M, scene.cur, np.int32), c(scene.pt_pos, np.float64)

    def outputs(n, fill):
        return dict(px=pad(c(scene.px_init, np.float64))[:n].copy(), ok=np.full(n, fill, np.int32), ref_obs=np.zeros(n, np.int32),
                    sl=np.zeros(n, np.int32), A=np.zeros((n, 4)), patches=np.zeros((n, 100), np.uint8))

    ref = outputs(M, 0)
    ws = np.full(emu.svo_hip_match_workspace_bytes(cap) + 256, 0xFF, np.uint8)   # (poisoned: NaN / -1 to whoever reads scratch it did not write)
    rc = emu.svo_hip_find_match_direct(C.byref(layout), ptr(store), C.byref(cam), C.byref(frames), M, ptr(cur), ptr(pos), ptr(obs_ptr), C.byref(obs),
                                       5, 10, ptr(ref["px"]), ptr(ref["ok"]), ptr(ref["ref_obs"]), ptr(ref["sl"]), ptr(ref["A"]), ptr(ref["patches"]),
                                       ptr(ws), C.c_size_t(ws.size), None)
    assert rc == 0, rc
    res = outputs(cap, -7)
    d_M = np.array([M], np.int32)
    ob_begin, ob_end, cur_p, pos_p = pad(obs_ptr[:-1].copy()), pad(obs_ptr[1:].copy()), pad(cur), pad(pos)
    rc = emu.svo_hip_find_match_direct_indirect(C.byref(layout), ptr(store), C.byref(cam), C.byref(frames), cap, ptr(d_M), ptr(cur_p), ptr(pos_p),
                                                ptr(ob_begin), ptr(ob_end), C.byref(obs), 5, 10, ptr(res["px"]), ptr(res["ok"]), ptr(res["ref_obs"]),
                                                ptr(res["sl"]), ptr(res["A"]), ptr(res["patches"]), ptr(ws), C.c_size_t(ws.size), None)
    assert rc == 0, rc
    for k in ref:
        assert np.array_equal(res[k][:M], ref[k]), k
    assert (res["ok"][M:] == -7).all() and ref["ok"].sum() > M // 2
    cell = (np.arange(M) // 3).astype(np.int32)
    cell_p = pad(cell)   # (kept in a name: a temporary would be gone before the call reads it)
    outs = []
    for indirect in (False, True):
        n, sel = np.zeros(1, np.int32), np.full(121, -1, np.int32)
        f, pos_o, lvl_o, has = np.zeros((121, 3)), np.zeros((121, 3)), np.zeros(121, np.int32), np.zeros(121, np.uint8)
        if indirect:
            rc = emu.svo_hip_select_matches_indirect(C.byref(cam), cap, ptr(d_M), ptr(cell_p), ptr(res["ok"]), ptr(res["px"]), ptr(res["sl"]),
                                                     ptr(pos_p), 120, ptr(n), ptr(sel), ptr(f), ptr(lvl_o), ptr(pos_o), ptr(has), None, 0, None)
        else:
            rc = emu.svo_hip_select_matches(C.byref(cam), M, ptr(cell), ptr(ref["ok"]), ptr(ref["px"]), ptr(ref["sl"]), ptr(pos), 120, ptr(n),
                                            ptr(sel), ptr(f), ptr(lvl_o), ptr(pos_o), ptr(has), None, 0, None)
        assert rc == 0, rc
        outs.append((n, sel, f, lvl_o, pos_o, has))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert outs[0][0][0] > 20
