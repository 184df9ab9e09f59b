"""svo_hip_frame_close (K11, csrc/frame_close.hip) of the host-emulated build (tests/emu_build.py: the kernel
compiled for the CPU through tests/host/hip_emu.h, one fiber per work-item, the LDS atomics as host atomics) on the cases of
tests/frame_close_cases.py against the sequential checker (tests/frame_close_checker.py): EVERY output bit for bit.  Every
output buffer lies between two guard bands and starts poisoned: whatever the entry defines it must write, and nothing else.
The bit comparison runs under all three schedules of the emulator (work-items in order, in reverse, wave by wave), each in a
process of its own because the schedule is read once per process.

Measured on the emulation: every output of all 34 batches has the checker's bits (largest difference 0) under the three
schedules."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import frame_close_cases as cases
import frame_close_checker as chk
from host_buffers import Guarded, compare_bits, ptr, same_bits
from rpg_svo_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRIES = ("svo_hip_frame_close", "svo_hip_frame_close_params_default")


@pytest.fixture(scope="module")
def emu():
    from emu_build import build_emulated
    return build_emulated((), bind=ENTRIES)


def call(emu, b, B=None, n_stride=None, kf_stride=None, grid=None, cells=None, override=(), drop_in=(), drop_out=()):
    """-> (return code, Guarded outputs)"""
    inp = cases.inputs(b)
    B = len(b.seqs) if B is None else B
    n_stride = b.n_stride if n_stride is None else n_stride
    kf_stride = b.kf_stride if kf_stride is None else kf_stride
    cell_size, n_cols, n_rows = b.grid if grid is None else grid
    cells = n_cols * n_rows if cells is None else cells
    out = Guarded(cases.out_shapes(max(B, 0), max(min(n_stride, b.n_stride), 0), max(cells, 0)))
    i = capi.FrameCloseIn(*[None if k in drop_in else ptr(inp[k]) for k in capi.FRAME_CLOSE_INPUTS])
    o = capi.FrameCloseOut(*[None if k in drop_out else out.ptr(k) for k in capi.FRAME_CLOSE_OUTPUTS])
    args = dict(cam=C.byref(capi.camera(b.cam)), inp=C.byref(i), params=C.byref(cases.params_struct(capi, b.params)), out=C.byref(o))
    args.update(dict(override))
    rc = emu.svo_hip_frame_close(args["cam"], B, n_stride, kf_stride, args["inp"], cell_size, n_cols, n_rows, cells, args["params"], args["out"], None)
    return rc, out


@pytest.mark.parametrize("name", cases.NAMES)
def test_frame_close_has_the_checkers_bits(emu, name):
    b = cases.batches()[name]
    rc, out = call(emu, b)
    assert rc == 0 and out.guards_intact()
    compare_bits(out.view, b.expect, name)   # (the outputs started poisoned: equal bits also mean every element was written)


def run_every_case():
    """(what the schedule test runs in a child process) -> the number of batches compared"""
    from emu_build import build_emulated
    emu = build_emulated((), bind=ENTRIES)
    for name in cases.NAMES:
        b = cases.batches()[name]
        rc, out = call(emu, b)
        assert rc == 0 and out.guards_intact(), name
        compare_bits(out.view, b.expect, name)
    return len(cases.NAMES)


@pytest.mark.parametrize("schedule", ["reverse", "waves"])
def test_the_schedule_of_the_work_items_does_not_matter(emu, schedule):
    env = dict(os.environ, SVO_EMU_SCHEDULE=schedule, PYTHONPATH=os.pathsep.join([HERE, os.path.dirname(HERE), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", "import test_frame_close_emulated as t; print('compared', t.run_every_case())"],
                       capture_output=True, text=True, env=env, cwd=HERE, timeout=900)
    assert r.returncode == 0 and f"compared {len(cases.NAMES)}" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_default_parameters(emu):
    p = capi.FrameCloseParams(1, 2, 3, 4, 5.0, 6, 7)
    assert emu.svo_hip_frame_close_params_default(C.byref(p)) == 0 and emu.svo_hip_frame_close_params_default(None) == -1
    assert {k: getattr(p, k) for k in chk.DEFAULTS} == chk.DEFAULTS and p.reserved == 0


def test_what_the_cases_cover():
    """(the properties the cases are there for, read off the checker's answers)"""
    B = cases.batches()
    assert list(B["gates"].expect["gate"]) == [1, 0, 2, 3, 0, 3, 0, 3, 3, 0]
    assert list(B["gates_low_min"].expect["gate"]) == [1, 0, 2, 0, 2]
    e = B["gates"].expect
    inp = cases.inputs(B["gates"])
    for k, g in enumerate(e["gate"]):
        assert same_bits(e["T_out"][k], inp["T_last" if g in (1, 3) else "T_f_w"][k])
        assert e["quality"][k] == (chk.TRACKING_INSUFFICIENT if g else chk.TRACKING_GOOD) and (e["result"][k] == chk.RESULT_FAILURE) == (g != 0)
    e = B["kf_box"].expect
    assert list(e["kf_block"]) == [-1, 0, -1, -1, 0, 0] * 3 and (e["depth_mean"] == 2.0).all() and (e["gate"] == 0).all()
    assert list(e["result"]) == [chk.RESULT_IS_KEYFRAME if k < 0 else chk.RESULT_NO_KEYFRAME for k in e["kf_block"]]
    assert list(B["furthest_3"].expect["kf_remove"]) == [-1, 0, 0, -1, 1] and (B["furthest_2"].expect["kf_remove"] == -1).all()
    e = B["every_exit"].expect
    assert list(e["gate"][:5]) == [0, 1, 2, 3, 0]
    assert list(e["result"][:5]) == [chk.RESULT_IS_KEYFRAME, chk.RESULT_FAILURE, chk.RESULT_FAILURE, chk.RESULT_FAILURE, chk.RESULT_NO_KEYFRAME]
    e = B["keyframes"].expect                      # n_kf 0, 1, 9, 10, 11, 64, 70 x overlap none, one, all
    assert (e["kf_block"][0::3] == -1).all() and (e["kf_block"] >= 0).any() and (e["kf_block"] > 0).any()
    assert (e["kf_remove"][:9] == -1).all() and (e["kf_remove"][9:] >= 0).all() and e["kf_remove"].max() > 10
    e = B["point_modes"].expect                    # none, all, alternating, first, last, random
    assert list(e["nobs_out"][:5]) == [0, 66, 33, 1, 1] and (e["key_pts"][0] == -1).all() and e["depth_mean"][0] == 0 and e["depth_min"][0] == 0
    assert (e["key_pts"][3][e["key_pts"][3] >= 0] == 0).all() and (e["key_pts"][4][e["key_pts"][4] >= 0] == 65).all()
    assert e["occupancy"][0].any()                 # rows without a point still occupy their cells
    e = B["rows65"].expect                         # n 0, 1, 49, 50, 63, 64, 65, 70 (clamped)
    assert list(e["valid"].sum(axis=1) == e["nobs_out"]) == [True] * 8 and e["nobs_out"][7] <= 65 and not e["occupancy"][0].any()
    assert (B["between_160x120"].expect["key_pts"][0, 1:] == -1).all() and B["between_160x120"].expect["key_pts"][0, 0] >= 0
    k = B["between_33x47"].expect["key_pts"][0]
    assert k[1] == k[4] and k[2] == k[3] and (k >= 0).all()
    for key in cases.CAMERAS:
        k = B[f"ties_{key}"].expect["key_pts"][0]
        assert (k < 50).all() and (k >= 0).all(), key
        b = B[f"centre_lines_{key}"]
        assert [int(v) for v in b.expect["key_pts"][:, 0]] == [s.centre_row for s in b.seqs]
        e = B[f"bad_pixels_{key}"].expect
        assert e["key_pts"][0, 0] == 0 and e["key_pts"][1, 0] not in (20, -1)      # a NaN first member stays; a later one is passed over
        assert np.isnan(B[f"bad_pixels_{key}"].seqs[0].px[0, 0]) and np.isfinite(B[f"bad_pixels_{key}"].seqs[1].px[e["key_pts"][1, 0]]).all()
        assert e["occupancy"][0, 0] == 1 and e["occupancy"][0, -1] == 1
    for n in cases.EQUAL_DEPTH_COUNTS:
        b = B[f"equal_depths_{n}"]
        z = np.sort(b.seqs[0].z_cam)
        assert b.expect["depth_mean"][0] == z[n // 2] and b.expect["depth_min"][0] == z[0] and b.expect["nobs_out"][0] == n
        assert n < 5 or z[n // 2 - 1] == z[n // 2] == z[n // 2 + 1]
    assert {int(s.T_f_w[0] + s.T_f_w[4] + s.T_f_w[8] > 0) for b in B.values() for s in b.seqs} == {0, 1}   # both quaternion branches


def test_identical_sequences_and_repeated_calls_give_the_same_bits(emu):
    b = cases.batches()["every_exit"]
    _, one = call(emu, b)
    _, two = call(emu, b)
    for k in one.view:
        assert same_bits(one.view[k], two.view[k]), k
        for i, j in ((0, 5), (0, 15), (2, 7), (4, 9), (3, 13)):
            assert same_bits(one.view[k][i], one.view[k][j]), (k, i, j)


def test_limits_and_error_codes(emu):
    b = cases.batches()["rows65"]
    cell_size, n_cols, n_rows = b.grid
    rc, out = call(emu, b, B=0)                                    # a successful no-op that touches nothing
    assert rc == 0 and out.untouched() and out.guards_intact()
    for kw in (dict(B=-1), dict(n_stride=-1), dict(kf_stride=-1)):
        assert call(emu, b, **kw)[0] == -1, kw
    assert call(emu, b, n_stride=1025)[0] == -2 and call(emu, b, kf_stride=65)[0] == -2
    for grid in ((0, n_cols, n_rows), (-1, n_cols, n_rows), (cell_size, -1, n_rows), (cell_size, n_cols, -1)):
        assert call(emu, b, grid=grid, cells=n_cols * n_rows)[0] == -1, grid
    for cells in (n_cols * n_rows - 1, n_cols * n_rows + 1, -1):
        assert call(emu, b, cells=cells)[0] == -1, cells
    for missing in ("cam", "inp", "params", "out"):
        rc, out = call(emu, b, override={missing: None})
        assert rc == -1 and out.untouched(), missing
    for k in capi.FRAME_CLOSE_INPUTS:
        rc, out = call(emu, b, drop_in=(k,))
        assert rc == -1 and out.untouched(), k
    for k in capi.FRAME_CLOSE_OUTPUTS:
        rc, out = call(emu, b, drop_out=(k,))
        assert rc == -1 and out.untouched(), k
