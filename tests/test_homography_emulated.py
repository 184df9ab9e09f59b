"""svo_hip_homography_init of the host-emulated build (tests/emu_build.py: homography_init.hip compiled for the
CPU through tests/host/hip_emu.h, one fiber per work-item, the wave exchanges as rendezvous) on the cases of
tests/homography_cases.py against the f64 checker (tests/homography_checker.py), by the rule homography_cases.py states.

Measured on the emulation (separate multiply and add): every discrete output equal in all 23 cases; the largest relative
difference of a continuous output is 2.95e-11 (point_w of case m64; 9.7e-12 on m65, below 7e-13 on every other case).
The two large ones are the refinement's stop rule, not arithmetic: near convergence a Gauss-Newton step changes the cost
in its last bits, so device and checker may keep one step more or less, and H then differs by the size of that step."""
import ctypes as C

import numpy as np
import pytest

import homography_cases as cases
from host_buffers import ptr, same_bits
from rpg_svo_amd import capi

# the largest relative difference to the checker of any continuous output over all cases, measured on the emulation
MEASURED_EMULATION = 2.95e-11
BOUND = 100 * MEASURED_EMULATION      # 2.95e-9 relative; the device test uses the same bound (never looser than 1e-6)


@pytest.fixture(scope="module")
def emu():
    from emu_build import build_emulated
    return build_emulated(())


def make_params(emu, **kw):
    p = capi.HomographyParams()
    assert emu.svo_hip_homography_params_default(C.byref(p)) == 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def call(emu, cam, inp, params, n_pairs=None, n_pts=None, poison=True, override=()):
    """-> (return code, name -> output array).  Outputs start poisoned: whatever the entry defines, it must write."""
    st = inp["status"]
    n_pairs = st.shape[0] if n_pairs is None else n_pairs
    n_pts = st.shape[1] if n_pts is None else n_pts
    outs = {}
    for k, (shape, dt) in cases.out_shapes(max(n_pairs, 1), max(n_pts, 1)).items():
        outs[k] = np.full(shape, 0x55 if np.issubdtype(dt, np.integer) else np.nan, dt) if poison else np.zeros(shape, dt)
    o = capi.HomographyOut(*[outs[k].ctypes.data for k in capi.HOMOGRAPHY_OUTPUTS])
    args = dict(cam=C.byref(capi.camera(cam)), f_ref=ptr(inp["f_ref"]), f_cur=ptr(inp["f_cur"]), status=ptr(st), px_ref=ptr(inp["px_ref"]),
                px_cur=ptr(inp["px_cur"]), T_ref_w=ptr(inp["T_ref_w"]), params=C.byref(params), out=C.byref(o))
    args.update(dict(override))
    rc = emu.svo_hip_homography_init(args["cam"], n_pairs, n_pts, args["f_ref"], args["f_cur"], args["status"], args["px_ref"],
                                     args["px_cur"], args["T_ref_w"], args["params"], args["out"], None)
    return rc, outs


@pytest.mark.parametrize("name", cases.NAMES)
def test_against_checker(emu, name):
    b = cases.batches()[name]
    rc, got = call(emu, b.cam, cases.inputs(b), make_params(emu, **b.params))
    assert rc == 0
    worst = cases.compare(b, got, BOUND)
    print(name, {k: f"{v:.2e}" for k, v in worst.items()})


def test_identical_pairs_and_repeated_calls_give_the_same_bits(emu):
    for name, twins in (("three_pairs", (0, 2)), ("five_pairs", (0, 4))):
        b = cases.batches()[name]
        p = make_params(emu, **b.params)
        _, one = call(emu, b.cam, cases.inputs(b), p)
        _, two = call(emu, b.cam, cases.inputs(b), p)
        assert all(same_bits(one[k], two[k]) for k in one)
        i, j = twins
        assert all(same_bits(v[i:i + 1], v[j:j + 1]) for v in one.values())


def test_limits_and_error_codes(emu):
    b = cases.batches()["m63"]
    inp = cases.inputs(b)
    p = make_params(emu)
    assert (p.reproj_thresh, p.map_scale, p.min_inliers, p.n_hypotheses, p.refine_iters, p.seed) == (2.0, 1.0, 40, 512, 10, 0)
    assert emu.svo_hip_homography_params_default(None) == -1
    assert call(emu, b.cam, inp, p, n_pts=0)[0] == 0 and call(emu, b.cam, inp, p, n_pairs=0)[0] == 0      # successful no-ops
    rc, untouched = call(emu, b.cam, inp, p, n_pairs=0)
    assert rc == 0 and np.isnan(untouched["H"]).all()
    assert call(emu, b.cam, inp, p, n_pts=-1)[0] == -1 and call(emu, b.cam, inp, p, n_pairs=-1)[0] == -1
    assert call(emu, b.cam, inp, p, n_pts=1025)[0] == -2
    for bad in (0, -1, 4097):
        assert call(emu, b.cam, inp, make_params(emu, n_hypotheses=bad))[0] == -2
    assert call(emu, b.cam, inp, make_params(emu, n_hypotheses=4096, refine_iters=0))[0] == 0
    assert call(emu, b.cam, inp, make_params(emu, refine_iters=-1))[0] == -1
    assert call(emu, b.cam, inp, make_params(emu, min_inliers=-1))[0] == -1
    assert call(emu, b.cam, inp, make_params(emu, reproj_thresh=0.0))[0] == -1
    assert call(emu, b.cam, inp, make_params(emu, reproj_thresh=float("nan")))[0] == -1
    for missing in ("cam", "f_ref", "f_cur", "status", "px_ref", "px_cur", "T_ref_w", "params", "out"):
        assert call(emu, b.cam, inp, p, override={missing: None})[0] == -1, missing
    for k in capi.HOMOGRAPHY_OUTPUTS:
        outs = {n: np.zeros(s, dt) for n, (s, dt) in cases.out_shapes(1, b.n_pts).items()}
        o = capi.HomographyOut(*[None if n == k else outs[n].ctypes.data for n in capi.HOMOGRAPHY_OUTPUTS])
        assert call(emu, b.cam, inp, p, override={"out": C.byref(o)})[0] == -1, k
    cam = cases.camera()
    cam.model = 7
    assert call(emu, cam, inp, p)[0] == -1


def test_lost_points_and_failed_pairs_hold_the_defined_zeros(emu):
    """(compare() checks the zeros of every case; here: from poisoned output buffers, for the pairs that fail at each step)"""
    for name, i, status, result in (("five_pairs", 1, 1, 0), ("five_pairs", 3, 1, 0), ("collinear", 0, 1, 0), ("identical_views", 0, 2, 0),
                                    ("too_few_inliers", 0, 0, 0)):
        b = cases.batches()[name]
        rc, got = call(emu, b.cam, cases.inputs(b), make_params(emu, **b.params))
        assert rc == 0 and got["status"][i] == status and got["result"][i] == result
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
        if name == "too_few_inliers":
            assert 0 < got["n_inliers"][i] < b.params["min_inliers"] and np.any(got["xyz_in_cur"][i]) and np.any(got["T_cur_from_ref"][i])
