"""svo_hip_homography_init on the device (through rpg_svo_amd.initialization.homography_init) on the cases of
tests/homography_cases.py -- the cases of tests/test_homography_emulated.py, here with the real wave exchanges, the real
LDS atomic and fused multiply-adds inside the hypothesis scores -- against the f64 checker (tests/homography_checker.py)
by the rule homography_cases.py states; the continuous bound is the emulated test's (100 x what the emulation measured).
Also: the same bits for identical pairs at different batch positions, for a repeated call and for a captured and
replayed HIP graph; the zeros of lost points and failed pairs from poisoned output buffers.

Measured on an MI355X: not yet -- every test prints its largest differences; the emulation's figures are in
tests/test_homography_emulated.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import homography_cases as cases
from host_buffers import same_bits
from test_homography_emulated import BOUND

pytestmark = pytest.mark.gpu


def run(dev, b, out=None, poison=True):
    from rpg_svo_amd import initialization as init
    inp = {k: torch.from_numpy(v).to(dev) for k, v in cases.inputs(b).items()}
    n, m = inp["status"].shape
    if out is None:
        out = init.homography_outputs(n, m, dev)
        if poison:   # whatever the entry defines, it must write
            for v in out.values():
                v.fill_(float("nan") if v.dtype == torch.float64 else 0x55)
    init.homography_init(b.cam, inp["f_ref"], inp["f_cur"], inp["status"], inp["px_ref"], inp["px_cur"], inp["T_ref_w"],
                         init.homography_params(**b.params), out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", cases.NAMES)
def test_against_checker(gpu_device, name):
    b = cases.batches()[name]
    got = run(gpu_device, b)
    worst = cases.compare(b, got, BOUND)
    print(name, {k: f"{v:.2e}" for k, v in worst.items()})


def test_identical_pairs_and_repeated_calls_give_the_same_bits(gpu_device):
    for name, (i, j) in (("three_pairs", (0, 2)), ("five_pairs", (0, 4))):
        b = cases.batches()[name]
        one, two = run(gpu_device, b), run(gpu_device, b)
        assert all(same_bits(one[k], two[k]) for k in one)
        assert all(same_bits(v[i:i + 1], v[j:j + 1]) for v in one.values())


def test_captured_and_replayed_graph_gives_the_same_bits(gpu_device):
    from rpg_svo_amd import capi, initialization as init
    b = cases.batches()["five_pairs"]
    direct = run(gpu_device, b)
    lib = capi.load()
    inp = {k: torch.from_numpy(v).to(gpu_device) for k, v in cases.inputs(b).items()}
    n, m = inp["status"].shape
    out = init.homography_outputs(n, m, gpu_device)
    o = capi.HomographyOut(*[out[k].data_ptr() for k in capi.HOMOGRAPHY_OUTPUTS])
    cam, params = capi.camera(b.cam), init.homography_params(**b.params)
    stream, graph = C.c_void_p(), C.c_void_p()
    capi.check(lib.svo_hip_stream_create(C.byref(stream)))
    torch.cuda.synchronize()
    try:
        capi.check(lib.svo_hip_graph_begin_capture(stream))
        capi.check(lib.svo_hip_homography_init(C.byref(cam), n, m, inp["f_ref"].data_ptr(), inp["f_cur"].data_ptr(), inp["status"].data_ptr(),
                                               inp["px_ref"].data_ptr(), inp["px_cur"].data_ptr(), inp["T_ref_w"].data_ptr(), C.byref(params),
                                               C.byref(o), stream))
        capi.check(lib.svo_hip_graph_end_capture(stream, C.byref(graph)))
        assert not any(bool(v.any()) for v in out.values())          # capturing ran nothing
        for _ in range(2):
            for v in out.values():
                v.fill_(float("nan") if v.dtype == torch.float64 else 0x55)
            torch.cuda.synchronize()
            capi.check(lib.svo_hip_graph_launch(graph, stream))
            capi.check(lib.svo_hip_stream_sync(stream))
            assert all(same_bits(direct[k], out[k].cpu().numpy()) for k in direct)
    finally:
        if graph:
            lib.svo_hip_graph_destroy(graph)
        lib.svo_hip_stream_destroy(stream)


def test_limits_and_error_codes(gpu_device):
    from rpg_svo_amd import capi, initialization as init
    b = cases.batches()["m63"]
    inp = {k: torch.from_numpy(v).to(gpu_device) for k, v in cases.inputs(b).items()}
    args = (b.cam, inp["f_ref"], inp["f_cur"], inp["status"], inp["px_ref"], inp["px_cur"], inp["T_ref_w"])
    for bad, code in ((dict(n_hypotheses=0), -2), (dict(n_hypotheses=4097), -2), (dict(refine_iters=-1), -1), (dict(reproj_thresh=0.0), -1)):
        with pytest.raises(capi.SvoHipError, match=f"code {code}"):
            init.homography_init(*args, init.homography_params(**bad))
    big = 1025
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=gpu_device)
    with pytest.raises(capi.SvoHipError, match="code -2"):
        init.homography_init(b.cam, z(1, big, 3), z(1, big, 3), z(1, big, dt=torch.uint8), z(1, big, 2, dt=torch.float32),
                             z(1, big, 2, dt=torch.float32), z(1, 12))
    out = init.homography_init(b.cam, z(0, 5, 3), z(0, 5, 3), z(0, 5, dt=torch.uint8), z(0, 5, 2, dt=torch.float32), z(0, 5, 2, dt=torch.float32), z(0, 12))
    assert out["result"].numel() == 0                                    # a successful no-op
    lib, o, p, cam = capi.load(), capi.HomographyOut(), init.homography_params(), capi.camera(b.cam)
    assert lib.svo_hip_homography_init(C.byref(cam), 1, b.n_pts, inp["f_ref"].data_ptr(), inp["f_cur"].data_ptr(), inp["status"].data_ptr(),
                                       inp["px_ref"].data_ptr(), inp["px_cur"].data_ptr(), inp["T_ref_w"].data_ptr(), C.byref(p), C.byref(o), None) == -1
    assert lib.svo_hip_homography_init(C.byref(cam), 1, b.n_pts, None, inp["f_cur"].data_ptr(), inp["status"].data_ptr(),
                                       inp["px_ref"].data_ptr(), inp["px_cur"].data_ptr(), inp["T_ref_w"].data_ptr(), C.byref(p), C.byref(o), None) == -1


def test_lost_points_and_failed_pairs_hold_the_defined_zeros(gpu_device):
    for name, i, status in (("five_pairs", 1, 1), ("five_pairs", 3, 1), ("collinear", 0, 1), ("identical_views", 0, 2), ("too_few_inliers", 0, 0)):
        b = cases.batches()[name]
        got = run(gpu_device, b)
        assert got["status"][i] == status and got["result"][i] == 0
        for k, v in got.items():
            assert np.isfinite(v[i]).all(), (name, k)
        lost = b.pairs[i].status == 0
        for k in ("inlier_H", "inlier", "point_ok", "xyz_in_cur", "point_w"):
            assert not np.any(got[k][i][lost]), (name, k)
        for k in ("depth_median", "scale", "T_cur_w", "point_w", "point_ok"):
            assert not np.any(got[k][i]), (name, k)
        if status == 1:
            assert got["best_hypothesis"][i] == -1
            for k in ("H", "n_inliers_H", "inlier_H", "T_cur_from_ref", "xyz_in_cur", "inlier", "n_inliers", "ambiguous"):
                assert not np.any(got[k][i]), (name, k)
        if status == 2:
            assert np.any(got["H"][i]) and got["n_inliers_H"][i] > 0
            for k in ("T_cur_from_ref", "xyz_in_cur", "inlier", "n_inliers", "ambiguous"):
                assert not np.any(got[k][i]), (name, k)
