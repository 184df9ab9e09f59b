"""TEST INFRASTRUCTURE, not a test.  The host-emulated library (tests/emu_build.py) behind the cases of tests/tracking_cases.py:
numpy buffers through the C ABI (host_buffers.ptr, the structs of rpg_svo_amd.capi), scratch poisoned with 0xFF plus 256 bytes
(NaN / -1 to whoever reads scratch it did not write).  Every function takes the emulated CDLL first and returns the numpy tuple
its twin in tests/tracking_device.py returns."""
import ctypes as C

import numpy as np

import tracking_cases as tc
from host_buffers import ptr
from rpg_svo_amd import capi


def pyramid_store(emu, images):
    n, h, w = images.shape
    layout = capi.pyr_layout(w, h, tc.N_LEVELS)
    buf = np.zeros(capi.pyr_store_bytes(layout, n), np.uint8)
    assert emu.svo_hip_pyramid_build_tiled(C.byref(layout), ptr(buf), 0, n, ptr(images), C.c_longlong(h * w), w, capi.HALFSAMPLE_AUTO, 0, None) == 0
    return layout, buf


def frame_table(T):
    slots = np.arange(T.shape[0], dtype=np.int32)
    fr = capi.Frames(T.shape[0], 0, slots.ctypes.data, T.ctypes.data)
    fr._keep = (slots, T)
    return fr


def store_and_frames(emu, c, T):
    """-> (pyramid layout, the store's bytes, svo_hip_frames over the poses T)"""
    # (the kernels only read the store: one per case and build)
    return c._memo(("emulated store", emu._name), lambda: pyramid_store(emu, c.images)) + (frame_table(np.ascontiguousarray(T)),)


def features(cols):
    return capi.Features(*[cols[k].ctypes.data for k in tc.FEATURE_KEYS])


def seeds(cols):
    return capi.Seeds(*[cols[k].ctypes.data for k in tc.SEED_KEYS])


def workspace(emu, n):
    emu.svo_hip_match_workspace_bytes.restype = C.c_size_t
    return np.full(emu.svo_hip_match_workspace_bytes(n) + 256, 0xFF, np.uint8)


def find_match_direct(emu, c):
    """-> ok, px, ref_obs, search level, A_cur_ref, patches"""
    s, P = c.scene, c.P
    layout, store, frames = store_and_frames(emu, c, c.T_match)
    obs, cam = features(c.obs_cols), capi.camera(s.cam)
    cur, pos, px = np.full(P, s.cur, np.int32), np.ascontiguousarray(s.pt_pos, dtype=np.float64), np.ascontiguousarray(s.px_init, dtype=np.float64).copy()
    ok, ref_obs, sl = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int32)
    A, patches = np.zeros((P, 4)), np.zeros((P, 100), np.uint8)
    ws = workspace(emu, P)
    rc = emu.svo_hip_find_match_direct(C.byref(layout), ptr(store), C.byref(cam), C.byref(frames), P, ptr(cur), ptr(pos), ptr(c.obs_ptr), C.byref(obs),
                                       tc.N_LEVELS, 10, ptr(px), ptr(ok), ptr(ref_obs), ptr(sl), ptr(A), ptr(patches), ptr(ws), C.c_size_t(ws.size), None)
    assert rc == 0, rc
    return ok, px, ref_obs, sl, A, patches


def find_epipolar(emu, c, q, align_1d, cap):
    """-> ok, depth, px_cur, search level"""
    layout, store, frames = store_and_frames(emu, c, c.T_f_w)
    ftr, cam = features(q.ftr_cols), capi.camera(c.scene.cam)
    cur = np.full(q.n, c.scene.cur, np.int32)
    de, dmin, dmax = (np.ascontiguousarray(x) for x in (q.d_est, q.d_min, q.d_max))
    o_ = capi.DepthFilterOptions(0, 0, 0.0, int(align_1d), 10, cap, 1, 1, tc.N_LEVELS, 0.7)
    ok, depth, px, lvl = np.zeros(q.n, np.int32), np.zeros(q.n), np.zeros((q.n, 2)), np.zeros(q.n, np.int32)
    ws = workspace(emu, q.n)
    rc = emu.svo_hip_find_epipolar_match_direct(C.byref(layout), ptr(store), C.byref(cam), C.byref(frames), q.n, ptr(cur), C.byref(ftr), ptr(de),
                                                ptr(dmin), ptr(dmax), C.byref(o_), ptr(ok), ptr(depth), ptr(px), ptr(lvl), ptr(ws), C.c_size_t(ws.size), None)
    assert rc == 0, rc
    return ok, depth, px, lvl


def _options(align_1d=0, subpix=1, cap=1000):
    return capi.DepthFilterOptions(3, 5, 200.0, int(align_1d), 10, cap, int(subpix), 1, tc.N_LEVELS, 0.7)


def _take(cols, idx):
    return {k: np.ascontiguousarray(v if idx is None else v[idx]) for k, v in cols.items()}


def update_seeds(emu, c, align_1d, subpix, cap, order=None):
    """order: the seeds in that order.  -> status, a, b, mu, sigma2, xyz, px_cur, z_range, batch_id"""
    P = c.P
    layout, store, frames = store_and_frames(emu, c, c.T_f_w)
    fc, st = _take(c.ftr_cols, order), {k: v.copy() for k, v in _take(c.seed_cols, order).items()}
    ftr, sd, cam, dopt = features(fc), seeds(st), capi.camera(c.scene.cam), _options(align_1d, subpix, cap)
    cur = np.full(P, c.scene.cur, np.int32)
    status, xyz, px = np.zeros(P, np.int32), np.zeros((P, 3)), np.zeros((P, 2))
    ws = workspace(emu, P)
    rc = emu.svo_hip_update_seeds(C.byref(layout), ptr(store), C.byref(cam), C.byref(frames), P, ptr(cur), C.byref(ftr), C.byref(sd), C.byref(dopt),
                                  ptr(status), ptr(xyz), ptr(px), ptr(ws), C.c_size_t(ws.size), None)
    assert rc == 0, rc
    return status, st["a"], st["b"], st["mu"], st["sigma2"], xyz, px, st["z_range"], st["batch_id"]


def update_seeds_resident(emu, c, slots, parts, by_pose=False):
    """The seeds patched into a store of 3 P slots in the instalments `parts` and updated through
    svo_hip_update_seeds_resident; by_pose: through svo_hip_update_seeds_resident_pose -- the current frame's pose by value,
    its row of the table poisoned (a host that uploaded the tables before the pose was known), and without a pose EINVAL.
    -> status, xyz, px_cur, state [4,P], the store's seed columns, the store's feature columns"""
    P, n_slots, cur = c.P, 3 * c.P, int(c.scene.cur)
    T = c.T_f_w.copy()
    if by_pose:
        T[cur] = np.nan
    layout, store, frames = store_and_frames(emu, c, T)
    fS = {k: np.full((n_slots,) + v.shape[1:], tc.FILL, v.dtype) for k, v in c.ftr_cols.items()}
    sS = {k: np.full(n_slots, tc.FILL, v.dtype) for k, v in c.seed_cols.items()}
    ftrS, sdS = features(fS), seeds(sS)
    for part in parts:
        fp, sp, sl = _take(c.ftr_cols, part), _take(c.seed_cols, part), np.ascontiguousarray(slots[part])
        patch = capi.SeedPatch(len(part), 0, sl.ctypes.data, features(fp), seeds(sp))
        assert emu.svo_hip_seed_store_patch(C.byref(patch), C.byref(ftrS), C.byref(sdS), None) == 0
    cam, dopt, ws = capi.camera(c.scene.cam), _options(), workspace(emu, P)
    st, xyz, px, state = np.zeros(P, np.int32), np.zeros((P, 3)), np.zeros((P, 2)), np.zeros((4, P), np.float32)
    head = (C.byref(layout), ptr(store), C.byref(cam), C.byref(frames), cur)
    tail = (P, ptr(slots), C.byref(ftrS), C.byref(sdS), C.byref(dopt), ptr(st), ptr(xyz), ptr(px), ptr(state), ptr(ws), C.c_size_t(ws.size), None)
    if by_pose:
        T_cur = np.ascontiguousarray(c.T_f_w[cur].copy())
        assert emu.svo_hip_update_seeds_resident_pose(*head, ptr(T_cur), *tail) == 0
        out = tuple(x.copy() for x in (st, xyz, px, state)) + ({k: v.copy() for k, v in sS.items()}, fS)
        assert emu.svo_hip_update_seeds_resident_pose(*head, None, *tail) == -1  # (EINVAL: no pose)
        return out
    assert emu.svo_hip_update_seeds_resident(*head, *tail) == 0
    return st, xyz, px, state, sS, fS


def pose_optimize(emu, cam, batch, n_iter, entry="", thresh=2.0):
    """entry: "", "_ordered" or "_deferred".  -> T, Cov, stats, ran, has_point"""
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
    n, f, level, pos = c(batch["n"], np.int32), c(batch["f"], np.float64), c(batch["level"], np.int32), c(batch["pos"], np.float64)
    B, ns = f.shape[0], f.shape[1]
    T, hpo = c(batch["T0"], np.float64).copy(), c(batch["hp"], np.uint8).copy()
    Cov, stats, ran = np.zeros((B, 36)), np.zeros((B, 4)), np.zeros(B, np.int32)
    cs = capi.camera(cam)
    rc = getattr(emu, "svo_hip_pose_optimize" + entry)(C.byref(cs), B, ptr(n), ns, ptr(f), ptr(level), ptr(pos), ptr(hpo), C.c_double(thresh), n_iter,
                                                       ptr(T), ptr(Cov), ptr(stats), ptr(ran), None)
    assert rc == 0, rc
    return T, Cov, stats, ran, hpo


def point_optimize(emu, T_f_w, obs_ptr, fr, ff, p0):
    frames, out = frame_table(np.ascontiguousarray(T_f_w)), p0.copy()
    assert emu.svo_hip_point_optimize(C.byref(frames), len(obs_ptr) - 1, ptr(obs_ptr), ptr(fr), ptr(ff), 5, ptr(out), None) == 0
    return out


def reproject_points(emu, scene):
    """-> cell, px of the scene's points in the current frame (cells of 30 px, 22 columns)"""
    frames, P = frame_table(np.ascontiguousarray(scene.T_f_w)), len(scene.pt_pos)
    cur, pos = np.full(P, scene.cur, np.int32), np.ascontiguousarray(scene.pt_pos, dtype=np.float64)
    cell, px = np.zeros(P, np.int32), np.zeros((P, 2))
    cs = capi.camera(scene.cam)
    assert emu.svo_hip_reproject_points(C.byref(cs), C.byref(frames), P, ptr(cur), ptr(pos), 30, 22, ptr(cell), ptr(px), None) == 0
    return cell, px


def select_matches(emu, cam, cell, ok, px, level, pos, max_fts):
    """-> n, sel, f, level, pos, has_point"""
    M, cs = len(cell), capi.camera(cam)
    cap = max(M, 1)
    n, sel, f = np.zeros(1, np.int32), np.zeros(cap, np.int32), np.zeros((cap, 3))
    lvl, p, has = np.zeros(cap, np.int32), np.zeros((cap, 3)), np.zeros(cap, np.uint8)
    rc = emu.svo_hip_select_matches(C.byref(cs), M, ptr(cell), ptr(ok), ptr(px), ptr(level), ptr(pos), max_fts, ptr(n), ptr(sel), ptr(f), ptr(lvl),
                                    ptr(p), ptr(has), None, 0, None)
    assert rc == 0, rc
    return n[0], sel, f, lvl, p, has


def update_seed_batch(emu, cols, x, tau2):
    """-> the seed columns after svo_hip_update_seed_batch"""
    cols = {k: v.copy() for k, v in cols.items()}
    ss = seeds(cols)
    assert emu.svo_hip_update_seed_batch(len(x), ptr(x), ptr(tau2), C.byref(ss), None) == 0
    return cols


def align_batch(emu, layout, store, tr, n_iter, entry="", extra=()):
    """svo_hip_align_batch<entry> on the trials tr (tracking_cases.align_trials).  -> px, ok, h_inv"""
    M = len(tr["slot"])
    px, ok, h_inv = tr["px0"].copy(), np.zeros(M, np.int32), np.zeros(M)
    rc = getattr(emu, "svo_hip_align_batch" + entry)(C.byref(layout), ptr(store), M, ptr(tr["slot"]), ptr(tr["level"]), ptr(tr["pwb"]), ptr(tr["dirs"]),
                                                     ptr(tr["use_1d"]), n_iter, ptr(px), ptr(ok), ptr(h_inv), *extra, None)
    assert rc == 0, (entry, rc)
    return px, ok, h_inv
