"""TEST INFRASTRUCTURE, not a test.  The device behind the cases of tests/tracking_cases.py: torch tensors through the Python
mirror rpg_svo_amd.tracking (which gets its coverage from these tests).  The functions of tests/tracking_emulated.py without the
CDLL argument, returning the same numpy tuples."""
import numpy as np
import torch

import tracking_cases as tc
from rpg_svo_amd import tracking
from rpg_svo_amd.pyramid import PyramidStore

DEVICE = "cuda:0"


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=DEVICE)


def host(ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


def store_and_frames(c, T):
    """-> (PyramidStore of the case's images, slot i = frame i; FrameTable over the poses T)"""
    n, h, w = c.images.shape
    store = PyramidStore(w, h, tc.N_LEVELS, n, device=DEVICE)
    store.load_images(torch.from_numpy(c.images).to(DEVICE))
    return store, tracking.FrameTable(torch.arange(n, dtype=torch.int32, device=DEVICE), dev(T, torch.float64))


def features(cols, idx=None):
    t = dict(frame=torch.int32, level=torch.int32, px=torch.float64, f=torch.float64, type=torch.uint8, grad=torch.float64)
    return tracking.FeatureSet(**{k: dev(cols[k] if idx is None else cols[k][idx], dt) for k, dt in t.items()})


def seeds(cols, idx=None):
    return tracking.SeedSet(**{k: dev(cols[k] if idx is None else cols[k][idx], torch.int32 if k == "batch_id" else torch.float32)
                               for k in tc.SEED_KEYS})


def _cur(c, n):
    return torch.full((n,), c.scene.cur, dtype=torch.int32, device=DEVICE)


def find_match_direct(c):
    """-> ok, px, ref_obs, search level, A_cur_ref, patches"""
    s = c.scene
    store, frames = store_and_frames(c, c.T_match)
    m = tracking.Matcher(align_max_iter=10, n_pyr_levels=tc.N_LEVELS)
    r = m.find_match_direct(store, s.cam, frames, _cur(c, c.P), dev(s.pt_pos, torch.float64), dev(c.obs_ptr, torch.int32), features(c.obs_cols),
                            dev(s.px_init, torch.float64))
    return host((r.ok, r.px_cur, r.ref_obs, r.search_level, r.A_cur_ref, r.patch_with_border))


def find_epipolar(c, q, align_1d, cap):
    """-> ok, depth, px_cur, search level"""
    store, frames = store_and_frames(c, c.T_f_w)
    return host(tracking.find_epipolar_match_direct(store, c.scene.cam, frames, _cur(c, q.n), features(q.ftr_cols), dev(q.d_est, torch.float64),
                                                    dev(q.d_min, torch.float64), dev(q.d_max, torch.float64), n_pyr_levels=tc.N_LEVELS,
                                                    align_1d=bool(align_1d), max_epi_search_steps=cap))


def update_seeds(c, align_1d, subpix, cap, order=None, cols=None):
    """order: the seeds in that order (an index may repeat); cols: other seed columns than the case's.
    -> status, a, b, mu, sigma2, xyz, px_cur"""
    store, frames = store_and_frames(c, c.T_f_w)
    fs, ss = features(c.ftr_cols, order), seeds(cols or c.seed_cols, order)
    df = tracking.DepthFilter(n_pyr_levels=tc.N_LEVELS, align_1d=bool(align_1d), subpix_refinement=bool(subpix), max_epi_search_steps=cap)
    status, xyz, px = df.update_seeds(store, c.scene.cam, frames, _cur(c, ss.mu.shape[0]), fs, ss, batch_counter=5)
    return host((status, ss.a, ss.b, ss.mu, ss.sigma2, xyz, px))


def update_seeds_resident(c, slots, parts):
    """The seeds patched into a store of 3 P slots in the instalments `parts` and updated through svo_hip_update_seeds_resident.
    -> status, xyz, px_cur, state [4,P], the store's seed columns, the store's feature columns"""
    n_slots = 3 * c.P
    store, frames = store_and_frames(c, c.T_f_w)
    z = lambda n, dt: torch.full((n,) if isinstance(n, int) else n, tc.FILL, dtype=dt, device=DEVICE)
    sf = tracking.FeatureSet(frame=z(n_slots, torch.int32), level=z(n_slots, torch.int32), px=z((n_slots, 2), torch.float64),
                             f=z((n_slots, 3), torch.float64), type=z(n_slots, torch.uint8), grad=z((n_slots, 2), torch.float64))
    sst = tracking.SeedSet(a=z(n_slots, torch.float32), b=z(n_slots, torch.float32), mu=z(n_slots, torch.float32), z_range=z(n_slots, torch.float32),
                           sigma2=z(n_slots, torch.float32), batch_id=z(n_slots, torch.int32))
    for part in parts:
        tracking.DepthFilter.seed_store_patch(dev(slots[part], torch.int32), features(c.ftr_cols, part), seeds(c.seed_cols, part), sf, sst)
    df = tracking.DepthFilter(n_pyr_levels=tc.N_LEVELS)
    out = host(df.update_seeds_resident(store, c.scene.cam, frames, c.scene.cur, dev(slots, torch.int32), sf, sst, batch_counter=5))
    return out + ({k: getattr(sst, k).cpu().numpy() for k in tc.SEED_KEYS}, {k: getattr(sf, k).cpu().numpy() for k in tc.FEATURE_KEYS})


def pose_optimize(cam, batch, n_iter, entry="", thresh=2.0):
    """entry: "", "_ordered" or "_deferred".  -> T, Cov, stats, ran, has_point"""
    r = tracking.optimize_gauss_newton(cam, dev(batch["n"], torch.int32), dev(batch["f"], torch.float64), dev(batch["level"], torch.int32),
                                       dev(batch["pos"], torch.float64), dev(batch["hp"], torch.uint8), dev(batch["T0"], torch.float64), thresh, n_iter,
                                       ordered=entry == "_ordered", deferred=entry == "_deferred")
    return host((r.T_f_w, r.Cov, r.stats, r.ran, r.has_point))


def point_optimize(T_f_w, obs_ptr, fr, ff, p0):
    n = len(T_f_w)
    frames = tracking.FrameTable(torch.arange(n, dtype=torch.int32, device=DEVICE), dev(T_f_w, torch.float64))
    return tracking.point_optimize(frames, dev(obs_ptr, torch.int32), dev(fr, torch.int32), dev(ff, torch.float64), dev(p0, torch.float64), 5).cpu().numpy()


def reproject_points(scene):
    """-> cell, px of the scene's points in the current frame (cells of 30 px, 22 columns)"""
    n, P = len(scene.T_f_w), len(scene.pt_pos)
    frames = tracking.FrameTable(torch.arange(n, dtype=torch.int32, device=DEVICE), dev(scene.T_f_w, torch.float64))
    return host(tracking.reproject_points(scene.cam, frames, torch.full((P,), scene.cur, dtype=torch.int32, device=DEVICE),
                                          dev(scene.pt_pos, torch.float64), 30, 22))


def select_matches(cam, cell, ok, px, level, pos, max_fts):
    """-> n, sel, f, level, pos, has_point"""
    out = host(tracking.select_matches(cam, dev(cell, torch.int32), dev(ok, torch.int32), dev(px, torch.float64), dev(level, torch.int32),
                                       dev(pos, torch.float64), max_fts))
    return (out[0][0],) + out[1:]


def update_seed_batch(cols, x, tau2):
    """-> the seed columns after svo_hip_update_seed_batch"""
    ss = seeds(cols)
    tracking.DepthFilter.update_seed(dev(x, torch.float32), dev(tau2, torch.float32), ss)
    torch.cuda.synchronize()
    return {k: getattr(ss, k).cpu().numpy() for k in tc.SEED_KEYS}


def align_batch(store, tr, n_iter, **kw):
    """tracking.align_batch on the trials tr (tracking_cases.align_trials).  -> px, ok, h_inv"""
    px = dev(tr["px0"], torch.float64)
    ok, h_inv = tracking.align_batch(store, dev(tr["slot"], torch.int32), dev(tr["level"], torch.int32), dev(tr["pwb"], torch.uint8), px, n_iter,
                                     dir=dev(tr["dirs"], torch.float32), use_1d=dev(tr["use_1d"], torch.uint8), **kw)
    return host((px, ok, h_inv))
