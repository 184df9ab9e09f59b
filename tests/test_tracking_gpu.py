"""GPU parity of the kernels behind rows a8-a13 (matcher / feature alignment / pose optimizer /
point optimizer / depth filter) against the oracle, through the C ABI.

The cases, the rules and their tolerances are those of tests/tracking_cases.py, which the host-emulated tests share
(tests/test_track_emulated.py, test_optimizers_emulated.py, test_entries_emulated.py); tests/tracking_device.py makes the
calls.  The float pipelines (feature alignment, affine warp) and every integer result (patch bytes, ZMSSD argmin, statuses,
pruning flags) are required to be IDENTICAL to the oracle's; f64 geometry carries the tolerance stated at its assert there.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import tracking_cases as tc
import tracking_device as td
from helpers import CAMERA_KINDS, camera_models, fuzz_rng
from oracle import pytrack
from rpg_svo_amd import capi, se3, tracking
from tracking_device import dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc(oracle, checker):
    """The CPU side of every comparison in this file: the C restatement and, where
    oracle/_ref/libsvo_ref.so is present, the reference's own translation units."""
    return pytrack.Track(checker)


@pytest.fixture(scope="module", params=CAMERA_KINDS)
def case(request):
    """the committed scene seen through each vikit camera model"""
    return tc.committed(request.param)


def _counted(store, tr, M, h_inv=True):
    """svo_hip_align_batch_counted on the first M trials -> px, ok, h_inv, evaluations"""
    px = dev(tr["px0"][:M], torch.float64)
    ok = torch.zeros(M, dtype=torch.int32, device="cuda:0")
    h = torch.zeros(M, dtype=torch.float64, device="cuda:0")
    ev = torch.zeros(M, dtype=torch.int32, device="cuda:0")
    keep = (dev(tr["slot"][:M], torch.int32), dev(tr["level"][:M], torch.int32), dev(tr["pwb"][:M], torch.uint8), dev(tr["dirs"][:M], torch.float32),
            dev(tr["use_1d"][:M], torch.uint8))
    capi.check(capi.load().svo_hip_align_batch_counted(C.byref(store.layout), store.ptr, M, keep[0].data_ptr(), keep[1].data_ptr(),
                                                       keep[2].data_ptr(), keep[3].data_ptr(), keep[4].data_ptr(), 10, px.data_ptr(), ok.data_ptr(),
                                                       h.data_ptr() if h_inv else None, ev.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return td.host((px, ok, h, ev))


def test_align_batch_bit_exact(gpu_device, orc, case):
    _, pyrs, _, _ = case.checker(orc.which)
    store, _ = td.store_and_frames(case, case.T_f_w)
    M, n_iter = 3000, 10
    tr = tc.align_trials(pyrs, fuzz_rng(3), M, 2.5)
    px, ok, h_inv = td.align_batch(store, tr, n_iter)
    assert tc.check_alignment(orc, pyrs, tr, n_iter, ok, px, h_inv) > M // 4


def test_wave_per_trial_alignment_is_the_lane_kernel_bit_for_bit(gpu_device, orc, case):
    """Batches of up to 8192 trials are aligned by one wave per trial (csrc/align_wave.h: a camera frame's trials), larger
    ones by one lane per trial (align_lanes.h).  The same 3000 trials alone (wave kernel) and as the head of a batch of
    9000 (lane kernel): verdicts, refined pixels, h_inv and evaluation counts identical in every bit.  Each kernel is
    pinned to the reference on its own: test_align_batch_bit_exact (3000 trials: the wave kernel), the full-size and
    phased tests (the lane kernel)."""
    store, _ = td.store_and_frames(case, case.T_f_w)
    M0, M1 = 3000, 9000
    tr = tc.align_trials(case.checker(orc.which)[1], fuzz_rng(23), M1, 4.0)
    wave = _counted(store, tr, M0)   # <= 8192 trials: the wave kernel
    lane = _counted(store, tr, M1)   # beyond: the lane kernel
    tc.same_alignment(wave, lane, M0)
    ok_w, ev_w = wave[1], wave[3]
    assert ok_w.sum() > M0 // 4 and (ev_w == 10).sum() > 50 and (tr["use_1d"][:M0] > 0).sum() > 500


def test_phased_alignment_is_the_single_launch_bit_for_bit(gpu_device, orc, case):
    """svo_hip_align_batch_phased (three launches, the unfinished trials compacted in between -- the form
    find_match_direct / update_seeds use for large batches) against the single launch on 73 728 trials: verdicts,
    refined pixels (bits), h_inv and evaluation counts identical.  The single launch itself is pinned to the
    reference by test_align_batch_bit_exact."""
    store, _ = td.store_and_frames(case, case.T_f_w)
    rng = fuzz_rng(11)
    M0, REP = 3072, 24
    tr = tc.align_trials(case.checker(orc.which)[1], rng, M0, 4.0)   # (starts far enough for many iterations)
    perm = rng.permutation(M0 * REP)  # copies of a trial land in different waves / queues
    tr = {k: np.ascontiguousarray(np.tile(a, (REP,) + (1,) * (a.ndim - 1))[perm]) for k, a in tr.items()}
    M = M0 * REP
    assert capi.load().svo_hip_align_workspace_bytes(M) > 0  # large enough for the phased path
    ev_b = torch.zeros(M, dtype=torch.int32, device="cuda:0")
    single = td.align_batch(store, tr, 10)
    phased = td.align_batch(store, tr, 10, phased=True, evaluations=ev_b)
    tc.same_alignment(phased, single)
    ev_a = _counted(store, tr, M, h_inv=False)[3]
    ev = ev_b.cpu().numpy()
    assert np.array_equal(ev_a, ev)
    assert (ev > 6).sum() > 100 and (ev <= 3).sum() > 100, np.bincount(ev)  # all three launches had work


def test_find_match_direct(gpu_device, orc, case):
    worst = tc.verify_matcher(case, *td.find_match_direct(case), which=orc.which)
    n_ok, n_edge = tc.matcher_coverage(case, orc.which)
    print(f"find_match_direct[{orc.which}]: max |dA_cur_ref| {worst:.2e}")
    assert n_ok > 200 and n_edge > 20


def test_reproject_points(gpu_device, orc, case):
    tc.check_reproject_points(orc, case.scene, *td.reproject_points(case.scene))


def test_pose_optimize_deferred(gpu_device, case):
    batch = tc.pose_deferred_batch(case.scene)
    tc.check_pose_deferred(batch, lambda n_iter, entry: td.pose_optimize(case.scene.cam, batch, n_iter, entry))


@pytest.mark.parametrize("ordered,row", [(True, 0), (False, 250), (False, 128), (False, 64)], ids=["ordered", "wave", "wave_rows_of_128", "wave_rows_of_64"])
def test_pose_optimize(gpu_device, orc, case, ordered, row):
    """ordered=True: the checker kernel (normal equations summed in the reference's order).  ordered=False: the pipeline's
    wave kernel on rows of 250, 128 and 64 observations.  The rule: tracking_cases.check_pose."""
    batch, want = case.pose_ref(orc.which, ordered, row)
    got = td.pose_optimize(case.scene.cam, batch, 10, "_ordered" if ordered else "")
    devs = tc.check_pose_batch(case.scene, batch, want, got, ordered)
    print(f"pose_optimize[{orc.which}, ordered={ordered}, row={row}]: max deviation over {len(devs)} frames of >= 20 live observations {max(devs):.2e}")


def test_point_optimize(gpu_device, orc, case):
    scene = case.scene
    obs_ptr, fr, ff, p0 = tc.point_optimize_inputs(scene)
    tc.check_point_optimize(orc, scene, obs_ptr, ff, p0, td.point_optimize(scene.T_f_w, obs_ptr, fr, ff, p0))


def test_find_epipolar_match_direct(gpu_device, orc, case):
    """Matcher::findEpipolarMatchDirect on its own (the seam matcher.h:113-123 offers besides the depth
    filter): verdict and search level identical, px_cur_ to 1e-9, depth to 1e-9 relative."""
    for align_1d in (0, 1):
        wpx, wd = tc.verify_epipolar(case, align_1d, 1000, *td.find_epipolar(case, case.epi, align_1d, 1000), which=orc.which)
        print(f"find_epipolar_match_direct[{orc.which}, align_1d={align_1d}]: max |dpx_cur| {wpx:.2e}, max relative depth difference {wd:.2e}")
        assert sum(r[0] for r in case.epi_ref(orc.which, align_1d)) > case.epi.n // 3


@pytest.mark.parametrize("cap", [6, 20])
def test_max_epi_search_steps_cap(gpu_device, orc, case, cap):
    """Matcher::Options::max_epi_search_steps below the scan length: tracking_cases.verify_epipolar_cap."""
    ok_free, *_ = td.find_epipolar(case, case.epi_cap, 0, 1000)
    tc.verify_epipolar_cap(case, cap, ok_free, *td.find_epipolar(case, case.epi_cap, 0, cap), which=orc.which)


def test_update_seeds_with_search_step_cap(gpu_device, orc, case):
    """DepthFilter::updateSeeds with Matcher::Options::max_epi_search_steps = 8: tracking_cases.verify_seeds_cap."""
    status_free, *_ = td.update_seeds(case, 0, 1, 1000)
    tc.verify_seeds_cap(case, 8, status_free, *td.update_seeds(case, 0, 1, 8), which=orc.which)


@pytest.mark.parametrize("align_1d,subpix", [(0, 1), (1, 1), (0, 0)])
def test_update_seeds(gpu_device, orc, case, align_1d, subpix):
    """subpix=0: Matcher::Options::subpix_refinement == false -- a scan match is triangulated straight
    from uv_best (matcher.cpp:316-318) instead of being refined by align1D/align2D.  In list order against the checker
    (tracking_cases.verify_seeds, the device's sigma2 rule), then keyframe by keyframe (seed_order): the same bits."""
    first = td.update_seeds(case, align_1d, subpix, 1000)
    w = tc.verify_seeds(case, align_1d, subpix, 1000, *first, which=orc.which, device=True)
    print(f"update_seeds[{orc.which}, align_1d={align_1d}, subpix={subpix}]: max relative deviation of a / b over "
          f"{w['n_ab']} compared seeds = {w['ab']:.3e}; sigma2: max relative {w['sigma2']:.3e}, "
          f"max in units of eps32 * mu^2 {w['s2_eps']:.2f}")
    tc.seed_coverage(case, orc.which, align_1d, subpix)
    order = tc.seed_order(case)
    tc.verify_seed_order(order, first, td.update_seeds(case, align_1d, subpix, 1000, order), which=orc.which)


def test_update_seeds_on_the_resident_store(gpu_device, case, orc):
    """Row N2, seeds: the seeds scattered over the slots of a resident store (svo_hip_seed_store_patch), updated through
    svo_hip_update_seeds_resident in list order: tracking_cases.verify_resident."""
    S = case.P
    st0, a, b, mu, s2, xyz0, px0 = td.update_seeds(case, 0, 1, 1000)
    slots = tc.resident_slots(case)
    resident = td.update_seeds_resident(case, slots, (np.arange(S // 2), np.arange(S // 2, S)))
    _, conv = tc.verify_resident(slots, 3 * S, (st0, xyz0, px0, dict(a=a, b=b, mu=mu, sigma2=s2)), resident)
    assert conv > 2


def test_large_batches_take_the_same_decisions(gpu_device, case, orc):
    """Batches of >= 65 536 trials run the alignment in phases inside svo_hip_find_match_direct / svo_hip_update_seeds,
    and the epipolar scan orders the seeds of a workgroup by length: the same trials, tiled and shuffled into a large
    batch, must come back with the results of the small batch (which the tests above pin to the reference)."""
    scene, P = case.scene, case.P
    store, frames = td.store_and_frames(case, case.T_match)
    rng = fuzz_rng(31)
    # -- findMatchDirect
    fs, ptr_s = td.features(case.obs_cols), case.obs_ptr
    m = tracking.Matcher(align_max_iter=10, n_pyr_levels=5)
    cur = lambda n: torch.full((n,), scene.cur, dtype=torch.int32, device="cuda:0")
    small = m.find_match_direct(store, scene.cam, frames, cur(P), dev(scene.pt_pos, torch.float64), dev(ptr_s, torch.int32), fs,
                                dev(scene.px_init, torch.float64))
    rep = 65536 // P + 2
    order = rng.permutation(P * rep) % P                       # trial k of the large batch is trial order[k] of the small one
    cnt = (ptr_s[1:] - ptr_s[:-1])[order]
    ptr_l = np.zeros(len(order) + 1, dtype=np.int32)
    ptr_l[1:] = np.cumsum(cnt)
    gather = np.concatenate([np.arange(ptr_s[i], ptr_s[i + 1]) for i in order])
    big = tracking.Matcher(align_max_iter=10, n_pyr_levels=5).find_match_direct(
        store, scene.cam, frames, cur(len(order)), dev(scene.pt_pos[order], torch.float64), dev(ptr_l, torch.int32),
        td.features(case.obs_cols, gather), dev(scene.px_init[order], torch.float64))
    torch.cuda.synchronize()
    oi = torch.as_tensor(order, device="cuda:0")
    assert torch.equal(big.ok, small.ok[oi]) and torch.equal(big.search_level, small.search_level[oi])
    assert np.array_equal(big.px_cur.cpu().numpy().view(np.uint64), small.px_cur[oi].cpu().numpy().view(np.uint64))
    assert torch.equal(big.patch_with_border, small.patch_with_border[oi])
    # -- updateSeeds (seeds of this test's own draws)
    S = P
    cols = tc.make_seeds(case.d_true, rng)
    small = td.update_seeds(case, 0, 1, 1000, np.arange(S), cols)
    order = rng.permutation(S * (65536 // S + 2)) % S
    large = td.update_seeds(case, 0, 1, 1000, order, cols)
    bits = lambda x: np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint32)
    for k in (0, 1, 2, 3, 4, 6):   # status, a, b, mu, sigma2, px_cur
        assert np.array_equal(bits(large[k]), bits(small[k][order])), k


def test_update_seed_batch(gpu_device, orc):
    seeds, cols, x, tau2 = tc.seed_batch(orc, fuzz_rng(6), 4000)
    tc.check_seed_batch(orc, seeds, x, tau2, td.update_seed_batch(cols, x, tau2))


@pytest.mark.parametrize("kind", CAMERA_KINDS)
def test_select_matches_like_the_cell_loop(gpu_device, kind):
    """svo_hip_select_matches against the restated cell loop of Reprojector::reprojectMap: tracking_cases.check_select_matches."""
    cam = camera_models()[kind]
    rng = fuzz_rng(77)
    for M, max_fts in tc.SELECT_SHAPES_DEVICE:
        trials = tc.select_trials(cam, rng, M)
        tc.check_select_matches(cam, trials, max_fts, *td.select_matches(cam, *trials, max_fts))


@pytest.mark.gpu
def test_frame_pose_compose_is_the_hosts_product(gpu_device):
    """svo_hip_frame_pose_compose on the device: the bits of the host's SE3(R, t) * T_ref (IEEE f64 division and square root,
    no contraction) and the host's ranking of the overlapping keyframes, which is what lets the drop-in verify a chain
    enqueued behind K1 (test_entries_emulated.py has the statement-level twin on the CPU)."""
    from rpg_svo_amd.pyramid import _stream_ptr
    lib = capi.load()
    rng = fuzz_rng(5)
    device = torch.device(gpu_device)
    td = lambda x, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device=device)
    for T, q, t in tc.frame_pose_compose_cases(rng, 256):
        dT, dq, dt = td(T), td(q), td(t)
        table = torch.zeros((3, 12), dtype=torch.float64, device=device)
        copy = torch.zeros(12, dtype=torch.float64, device=device)
        out = torch.zeros(12, dtype=torch.float64, device=device)
        sig = torch.zeros(1, dtype=torch.int32, device=device)
        capi.check(lib.svo_hip_frame_pose_compose(dT.data_ptr(), dq.data_ptr(), dt.data_ptr(), table.data_ptr(), 1, copy.data_ptr(),
                                                  out.data_ptr(), None, 0, 0, None, None, 0, None, None, sig.data_ptr(), 7,
                                                  _stream_ptr(device)), "svo_hip_frame_pose_compose")
        torch.cuda.synchronize()
        want = tc.host_frame_pose(T, q, t)
        assert np.array_equal(table[1].cpu().numpy(), want) and np.array_equal(copy.cpu().numpy(), want)
        assert np.array_equal(out.cpu().numpy(), want) and int(sig[0]) == 7
    cam = camera_models()["pinhole"]
    cs = capi.camera(cam)
    for trial in range(60):
        table, key_pos, key_valid = tc.keyframe_rank_case(rng)
        n_tab, n_kf = len(table), len(key_pos)
        T = np.ascontiguousarray(se3.exp(rng.normal(size=6) * 0.05)); q = rng.normal(size=4); q /= np.linalg.norm(q); t = rng.normal(size=3) * 0.2
        for max_n in (3, 10):
            tab = td(table); rank = torch.full((n_tab,), 99, dtype=torch.int32, device=device); rank2 = rank.clone()
            dT, dq, dt, kp, kv = td(T), td(q), td(t), td(key_pos), td(key_valid, torch.uint8)
            capi.check(lib.svo_hip_frame_pose_compose(dT.data_ptr(), dq.data_ptr(), dt.data_ptr(), tab.data_ptr(), n_tab - 2, None, None,
                                                      C.byref(cs), n_tab, n_kf, kp.data_ptr(), kv.data_ptr(), max_n, rank.data_ptr(),
                                                      rank2.data_ptr(), None, 0, _stream_ptr(device)), "svo_hip_frame_pose_compose")
            torch.cuda.synchronize()
            want = tc.host_keyframe_ranks(cam, tc.host_frame_pose(T, q, t), tc.composed_quat(T, q), key_pos, key_valid, tab.cpu().numpy(), n_kf, max_n)
            assert np.array_equal(rank.cpu().numpy(), want) and np.array_equal(rank2.cpu().numpy(), want), (trial, rank, want)
