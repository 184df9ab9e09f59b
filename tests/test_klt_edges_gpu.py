"""svo_hip_klt_track and svo_hip_klt_summarize on the device on the inputs of tests/klt_edge_cases.py -- the cases of
tests/test_klt_edges_emulated.py, here with fused multiply-adds, the real v_alignbyte and the real wave exchanges:
windows over every border and corner of small and odd-sized levels, both loaders of klt_track.hip and the switch between
them, the bounds rule at its exact limits, hostile initial flow, every parameter away from its default, coarse levels
skipped by the min-eigenvalue rule, batch indexing with and without the XCD remapping of workgroup ids, and the summary
step at the sizes and parities of its loops.  Against the f64 checker (tests/klt_checker.py), by the rule
klt_edge_cases.py states: status equal on every compared point, px_cur within 5e-3 px, error within 1e-2 grey levels,
only points on which the checker itself is ill-conditioned left out (none is, on these inputs); the summary bit for bit.

Measured on an MI355X: not yet -- every test prints its status differences and its largest position and error
difference; the emulation's figures are in tests/test_klt_edges_emulated.py."""
import numpy as np
import pytest
import torch

import klt_edge_cases as cases
from helpers import camera_models, CAMERA_KINDS
from test_klt_gpu import make_store

pytestmark = pytest.mark.gpu


def run(dev, c):
    from rpg_svo_amd.initialization import klt_params, klt_track
    store = make_store(c.images, dev, cases.N_LEVELS)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    p = klt_params()
    p.max_level, p.max_iter, p.eps, p.min_eig_threshold = c.params["max_level"], c.params["max_iter"], c.params["eps"], c.params["min_eig_threshold"]
    px_cur, status, error = t(c.px_in, torch.float32), t(c.st_in, torch.uint8), t(c.err_in, torch.float32)
    out = klt_track(store, t(c.ref_slot, torch.int32), t(c.cur_slot, torch.int32), t(c.px_ref, torch.float32), px_cur, status, error, p)
    torch.cuda.synchronize()
    assert out is error
    return px_cur.cpu().numpy(), status.cpu().numpy(), error.cpu().numpy()


@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_border_grid(gpu_device, oracle, size):
    c = cases.case_a(oracle, size)
    cases.verify_track(c, *run(gpu_device, c))


@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_loss_and_hostile_initial_flow(gpu_device, oracle, size):
    c = cases.case_b(oracle, size)
    cases.verify_track(c, *run(gpu_device, c))


@pytest.mark.parametrize("max_level", [4, 0])
@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bounds_rule_without_iterations(gpu_device, oracle, size, max_level):
    c = cases.case_c(oracle, size, max_level)
    cases.verify_bounds(c, *run(gpu_device, c))


@pytest.mark.parametrize("params", cases.PARAM_SETS, ids=lambda p: "-".join(f"{k}={v}" for k, v in p.items()))
@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_parameters(gpu_device, oracle, size, params):
    c = cases.case_a(oracle, size, **params)
    cases.verify_track(c, *run(gpu_device, c))


@pytest.mark.parametrize("kind", cases.E_KINDS)
def test_min_eig_rule_skips_coarse_levels(gpu_device, oracle, kind):
    c = cases.case_e(oracle, kind)
    cases.verify_track(c, *run(gpu_device, c))


@pytest.mark.parametrize("n_pairs,n_pts", [(3, 5), (4, 6)])
def test_batch_indexing(gpu_device, oracle, n_pairs, n_pts):
    """15 workgroups (xcd_contiguous_block is the identity) and 24 (dealt round the 8 XCDs)"""
    c = cases.case_f(oracle, n_pairs, n_pts)
    cases.verify_batch(c, *run(gpu_device, c))


@pytest.mark.parametrize("n_pts", cases.SUMMARY_SIZES)
@pytest.mark.parametrize("kind", CAMERA_KINDS)
def test_summary_sizes_and_parities(gpu_device, kind, n_pts):
    import ctypes as C
    from rpg_svo_amd import capi
    from rpg_svo_amd.tracking import cam2world
    cam = camera_models()[kind]
    px_ref, px_cur, st = cases.summary_case(n_pts)
    n_pairs = len(st)
    t = lambda a: torch.from_numpy(a).to(gpu_device)
    d_ref, d_cur, d_st = t(px_ref), t(px_cur), t(st)
    f = torch.full((n_pairs, n_pts, 3), float("nan"), dtype=torch.float64, device=gpu_device)
    d = torch.full((n_pairs, n_pts), float("nan"), dtype=torch.float64, device=gpu_device)
    n = torch.full((n_pairs,), -1, dtype=torch.int32, device=gpu_device)
    med = torch.full((n_pairs,), float("nan"), dtype=torch.float64, device=gpu_device)
    ccam = capi.camera(cam)
    capi.check(capi.load().svo_hip_klt_summarize(C.byref(ccam), n_pairs, n_pts, d_ref.data_ptr(), d_cur.data_ptr(), d_st.data_ptr(),
                                                 f.data_ptr(), d.data_ptr(), n.data_ptr(), med.data_ptr(), None), "svo_hip_klt_summarize")
    f_ref = cam2world(cam, d_cur.to(torch.float64).reshape(-1, 2)).reshape(n_pairs, n_pts, 3)
    torch.cuda.synchronize()
    cases.verify_summary(px_ref, px_cur, st, f.cpu().numpy(), d.cpu().numpy(), n.cpu().numpy(), med.cpu().numpy(), f_ref.cpu().numpy())
