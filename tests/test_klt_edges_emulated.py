"""svo_hip_klt_track and svo_hip_klt_summarize of the host-emulated build (tests/emu_build.py) on the inputs of
tests/klt_edge_cases.py: windows over every border and corner of small and odd-sized levels, both loaders of
klt_track.hip and the switch between them, the bounds rule at its exact limits, hostile initial flow, every parameter away
from its default, coarse levels skipped by the min-eigenvalue rule, batch indexing, and the summary step at the sizes
and parities of its loops -- against the f64 checker (tests/klt_checker.py), by the rule klt_edge_cases.py states: status
equal on every compared point, px_cur within 5e-3 px, error within 1e-2 grey levels, and only points on which the
checker itself is ill-conditioned left out (none is, on these inputs).

Measured on the emulation (separate multiply and add): no status differs and no point is left out in any case; largest
position difference 1.7e-5 px (150 x 118, eps 0 / max_iter 7), largest error difference 5.9e-5 grey levels (batch case); with
no iteration (bounds case) px_cur is the input's bits and the error differs by at most 1.9e-6.
Run under scripts/emu_sanitize.sh address as well: the border cases are where a read outside the store would show."""
import ctypes as C

import numpy as np
import pytest

import klt_edge_cases as cases
from helpers import camera_models, CAMERA_KINDS
from host_buffers import ptr
from rpg_svo_amd import capi
from test_klt_emulated import build_store, default_params, klt_track


@pytest.fixture(scope="module")
def emu():
    from emu_build import build_emulated
    return build_emulated(())


def run(emu, c):
    layout, store = build_store(emu, c.images, cases.N_LEVELS)
    p = default_params(emu)
    p.max_level, p.max_iter, p.eps, p.min_eig_threshold = c.params["max_level"], c.params["max_iter"], c.params["eps"], c.params["min_eig_threshold"]
    return klt_track(emu, layout, store, c.ref_slot, c.cur_slot, c.px_ref, c.px_in, c.st_in, error=c.err_in, params=p)


@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_border_grid(emu, oracle, size):
    c = cases.case_a(oracle, size)
    cases.verify_track(c, *run(emu, c))


@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_loss_and_hostile_initial_flow(emu, oracle, size):
    c = cases.case_b(oracle, size)
    cases.verify_track(c, *run(emu, c))


@pytest.mark.parametrize("max_level", [4, 0])
@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bounds_rule_without_iterations(emu, oracle, size, max_level):
    c = cases.case_c(oracle, size, max_level)
    cases.verify_bounds(c, *run(emu, c))


@pytest.mark.parametrize("params", cases.PARAM_SETS, ids=lambda p: "-".join(f"{k}={v}" for k, v in p.items()))
@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_parameters(emu, oracle, size, params):
    c = cases.case_a(oracle, size, **params)
    cases.verify_track(c, *run(emu, c))


@pytest.mark.parametrize("kind", cases.E_KINDS)
def test_min_eig_rule_skips_coarse_levels(emu, oracle, kind):
    c = cases.case_e(oracle, kind)
    cases.verify_track(c, *run(emu, c))


@pytest.mark.parametrize("n_pairs,n_pts", [(3, 5), (4, 6)])
def test_batch_indexing(emu, oracle, n_pairs, n_pts):
    """15 workgroups (xcd_contiguous_block is the identity) and 24 (dealt round the 8 XCDs)"""
    c = cases.case_f(oracle, n_pairs, n_pts)
    cases.verify_batch(c, *run(emu, c))


@pytest.mark.parametrize("n_pts", cases.SUMMARY_SIZES)
@pytest.mark.parametrize("kind", CAMERA_KINDS)
def test_summary_sizes_and_parities(emu, kind, n_pts):
    ccam = capi.camera(camera_models()[kind])
    px_ref, px_cur, st = cases.summary_case(n_pts)
    n_pairs = len(st)
    f, d = np.full((n_pairs, n_pts, 3), np.nan), np.full((n_pairs, n_pts), np.nan)
    n, med = np.full(n_pairs, -1, np.int32), np.full(n_pairs, np.nan)
    assert emu.svo_hip_klt_summarize(C.byref(ccam), n_pairs, n_pts, ptr(px_ref), ptr(px_cur), ptr(st), ptr(f), ptr(d), ptr(n), ptr(med), None) == 0
    f_ref = np.zeros((n_pairs, n_pts, 3))
    px64 = np.ascontiguousarray(px_cur.reshape(-1, 2).astype(np.float64))
    assert emu.svo_hip_cam2world(C.byref(ccam), n_pairs * n_pts, ptr(px64), ptr(f_ref), None) == 0
    cases.verify_summary(px_ref, px_cur, st, f, d, n, med, f_ref)
