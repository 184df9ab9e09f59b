"""BASELINE.json full-size configurations, checked through size-independent properties (the
oracle only sees a bounded sample): determinism, independence of a problem from the batch it
travels in, invariance to the order of the patches, zero-motion fixed point, recovery of the
ground-truth motion; plus parity at configs[1] / configs[3] / configs[4] shapes against BOTH checkers (the C
restatement and the reference's own SparseImgAlign translation unit, `checker` fixture): the reference sees the
1000-patch frames and the rig shape too."""
import numpy as np
import pytest
import torch

import k1_cases as k1
import k1_device
from helpers import make_batch, run_hip
from rpg_svo_amd import se3

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def big_vga(gpu_device):
    """configs[1] at bench scale: 2048 replay pairs, 640x480, 4 levels, 200 patches."""
    return k1.seq_bench(gpu_device)


def test_config1_bench_scale_properties(oracle, gpu_device, big_vga, checker):
    B = 2048
    b = make_batch(big_vga, [(i, i + 1) for i in range(B)], 4)
    T1, out1, _ = run_hip(b, 3, 0)
    T2, out2, _ = run_hip(b, 3, 0)
    # (1) deterministic: same launch twice, bit-identical poses and counters
    assert np.array_equal(T1, T2) and torch.equal(out1.iters, out2.iters) and torch.equal(out1.n_tracked, out2.n_tracked)
    # (2) every problem solved: all patches tracked, ground-truth motion recovered
    assert (out1.n_tracked.cpu().numpy() == 200).all()
    err = se3.log_norm(T1, b.T_gt_w)
    assert np.median(err) < 1.5e-4 and err.max() < 2e-3
    # (3) a problem does not depend on its batch: singles == members of the big launch, to the bit
    for i in (0, 777, 2047):
        bi = make_batch(big_vga, [(i, i + 1)], 4)
        Ti, outi, _ = run_hip(bi, 3, 0)
        assert np.array_equal(Ti[0], T1[i]) and torch.equal(outi.iters[0], out1.iters[i])
    # (4) oracle parity on a bounded sample of the same launch
    sample = k1.case("config1_sample")
    sample.built(seq=big_vga)
    k1.verify_pair(oracle, k1.DEV, sample.name, sample.schedules[0], k1_device.answer(T1, out1).rows(slice(None, None, 32)), which=checker)


def test_patch_order_invariance(gpu_device, big_vga):
    """Permuting Frame::fts_ only changes the summation tree: poses agree to rounding."""
    B = 256
    b = make_batch(big_vga, [(i, i + 1) for i in range(B)], 4)
    T1, out1, _ = run_hip(b, 3, 0)
    rng = np.random.default_rng(0)
    perm = rng.permutation(200)
    b.px, b.f, b.pos, b.has_point = b.px[:, perm], b.f[:, perm], b.pos[:, perm], b.has_point[:, perm]
    T2, out2, _ = run_hip(b, 3, 0)
    d = se3.log_norm(T1, T2)
    assert np.median(d) < 1e-7 and d.max() <= 1e-4  # f32 partial sums: ~1e-8, like the distance to the oracle
    assert (out1.iters == out2.iters).all(dim=1).float().mean() > 0.97


def test_zero_motion_fixed_point_at_scale(gpu_device, big_vga):
    B = 1024
    b = make_batch(big_vga, [(i, i) for i in range(B)], 4)  # cur == ref, prior == truth
    T, out, _ = run_hip(b, 3, 0)
    assert se3.log_norm(T, b.T_ref_w).max() < 1e-9
    assert (out.n_tracked.cpu().numpy() == 200).all()
    assert (out.iters.cpu().numpy()[:, :4] <= 2).all()  # first step is ~0: chi2 cannot improve


def test_config3_xga5_n1000_parity(oracle, gpu_device, checker):
    """configs[3] shape: 1280x960, 5 levels (4->0), 1000 patches per frame (1024-lane workgroups)."""
    c = k1.case("config3")
    b, schedule = c.built(device=gpu_device)[0], c.schedules[0]
    # svo_hip_sparse_align splits such a frame (> 512 patches, a batch of <= 128 frames) over FOUR workgroups of 256
    # lanes on one XCD that exchange their sums through its L2; svo_hip_sparse_align_workgroup keeps the frame on one
    # workgroup of 1024 lanes.  Both against the checker, and against each other: the same iteration counts and tracked
    # patches, poses to rounding (the sums are formed in a different order).
    split, one = k1_device.run(c, schedule), k1_device.run(c, schedule, "workgroup")
    for backend, answer in ((k1.DEV, split), (k1.DEV_WG, one)):
        k1.verify_pair(oracle, backend, c.name, schedule, answer, which=checker)
        assert (answer.status == 0).all()
    assert se3.log_norm(split.pose, b.T_gt_w)[[0, 1, 3, 4, 7]].max() < 5e-4
    k1.verify_split(split, one)


def test_config4_rig_752_default_schedule_parity(oracle, gpu_device, checker):
    """configs[4] shape: 752x480 cameras, reference default schedule (levels 4->2), 64 frames."""
    c = k1.case("config4")
    c.built(device=gpu_device)
    k1.verify_pair(oracle, k1.DEV, c.name, c.schedules[0], k1_device.run(c, c.schedules[0]), which=checker)


def test_store_beyond_4gib_addresses_correctly(gpu_device, big_vga):
    """A pyramid store of 11 000 VGA slots (4.55 GB): slots above the 4 GiB mark must behave exactly
    like slots 0/1 (64-bit slot offsets in every kernel that touches the store)."""
    from rpg_svo_amd.pyramid import PyramidStore
    from rpg_svo_amd.sparse_img_align import SparseImgAlign, marshal_problem
    from rpg_svo_amd import tracking
    n_slots = 11000
    store = PyramidStore(640, 480, 4, n_slots, device=gpu_device)
    assert store.buf.numel() > (1 << 32)
    imgs = big_vga.images[:2].to(gpu_device)
    store.load_images(imgs, first_slot=0)
    store.load_images(imgs, first_slot=n_slots - 2)
    for l in range(4):
        assert np.array_equal(store.level(0, l), store.level(n_slots - 2, l))
        assert np.array_equal(store.level(1, l), store.level(n_slots - 1, l))
    b = make_batch(big_vga, [(0, 1)], 4)
    T_cr, xyz = marshal_problem(b.T_ref_w, b.T_cur_w, b.f, b.pos)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=gpu_device)
    sia = SparseImgAlign(3, 0, 30)
    outs = []
    for ref, cur in ((0, 1), (n_slots - 2, n_slots - 1)):
        o = sia.run(store, b.cam, t([ref], torch.int32), t([cur], torch.int32), t(b.n, torch.int32), t(b.px, torch.float64),
                    t(xyz, torch.float64), t(T_cr, torch.float64))
        outs.append((o.T_cur_from_ref.cpu().numpy(), o.iters.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    # the detector and the matcher front end read the store too
    from rpg_svo_amd.feature_detection import FastDetector
    det = FastDetector(640, 480, 30, 3)
    a = det.detect(store, t([0, n_slots - 2], torch.int32), 20.0)
    assert torch.equal(a[0][0], a[0][1]) and torch.equal(a[2][0], a[2][1])
    pwb = torch.randint(0, 256, (64, 100), dtype=torch.uint8, device=gpu_device)
    px0 = torch.rand(64, 2, dtype=torch.float64, device=gpu_device) * 200 + 100
    res = []
    for s in (1, n_slots - 1):
        px = px0.clone()
        ok, _ = tracking.align_batch(store, torch.full((64,), s, dtype=torch.int32, device=gpu_device),
                                     torch.zeros(64, dtype=torch.int32, device=gpu_device), pwb, px, 10)
        res.append((px.cpu().numpy(), ok.cpu().numpy()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
