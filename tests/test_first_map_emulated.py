"""svo_hip_first_map and svo_hip_initialize_seeds (K10, csrc/first_map.hip) of the host-emulated build
(tests/emu_build.py: the kernels compiled for the CPU through tests/host/hip_emu.h, one fiber per work-item, the
LDS atomics as host atomics) on the cases of tests/first_map_cases.py against the sequential checker
(tests/first_map_checker.py): EVERY output bit for bit.  Every output buffer lies between two guard bands and starts
poisoned: whatever the entry defines it must write, and nothing else.

Measured on the emulation: every output of all 32 first-map batches and all 10 seed cases has the checker's bits (largest
difference 0); also with the work-items scheduled in reverse and wave by wave (SVO_EMU_SCHEDULE=reverse / waves)."""
import ctypes as C

import numpy as np
import pytest

import first_map_cases as cases
import first_map_checker as chk
from host_buffers import Guarded, compare_bits, ptr, same_bits
from rpg_svo_amd import capi


@pytest.fixture(scope="module")
def emu():
    from emu_build import build_emulated
    return build_emulated((), bind=("svo_hip_first_map", "svo_hip_initialize_seeds"))   # (the cases pass addresses as ints, which need the argtypes)


def call_first_map(emu, b, n_seq=None, n_pts=None, override=(), grid=None, cells=None):
    """-> (return code, Guarded outputs)"""
    inp = cases.inputs(b)
    n_seq = len(b.seqs) if n_seq is None else n_seq
    n_pts = b.n_pts if n_pts is None else n_pts
    cell_size, n_cols, n_rows = b.grid if grid is None else grid
    cells = n_cols * n_rows if cells is None else cells
    out = Guarded(cases.out_shapes(max(n_seq, 0), max(n_pts, 0), max(cells, 0)))
    o = capi.FirstMapOut(*[out.ptr(k) for k in capi.FIRST_MAP_OUTPUTS])
    args = dict(cam=C.byref(capi.camera(b.cam)), out=C.byref(o), **{k: ptr(inp[k]) for k in cases.INPUTS})
    args.update(dict(override))
    rc = emu.svo_hip_first_map(args["cam"], n_seq, n_pts, *[args[k] for k in cases.INPUTS], cell_size, n_cols, n_rows, cells, args["out"], None)
    return rc, out


def call_seeds(emu, c, stride, batch_id, n_frames=None, n_cells=None, override=(), optional=True):
    n_frames = c.n_frames if n_frames is None else n_frames
    n_cells = c.n_cells if n_cells is None else n_cells
    out = Guarded(chk.seed_out_shapes(max(n_frames, 0), max(stride, 0)))
    o = capi.SeedInitOut(*[out.ptr(k) if optional or k not in ("type", "grad") else None for k in capi.SEED_INIT_OUTPUTS])
    args = dict(cam=C.byref(capi.camera(c.cam)), xy=ptr(c.xy), level=ptr(c.level), score=ptr(c.score), frame_index=ptr(c.frame_index),
                depth_mean=ptr(c.depth_mean), depth_min=ptr(c.depth_min), out=C.byref(o))
    args.update(dict(override))
    rc = emu.svo_hip_initialize_seeds(args["cam"], n_frames, n_cells, args["xy"], args["level"], args["score"], c.threshold, args["frame_index"],
                                      args["depth_mean"], args["depth_min"], batch_id, stride, args["out"], None)
    return rc, out


@pytest.mark.parametrize("name", cases.NAMES)
def test_first_map_has_the_checkers_bits(emu, name):
    b = cases.batches()[name]
    rc, out = call_first_map(emu, b)
    assert rc == 0 and out.guards_intact()
    compare_bits(out.view, b.expect, name)   # (the outputs started poisoned: equal bits also mean every element was written)


def test_what_the_cases_cover():
    """(the properties the cases are there for, read off the checker's answers)"""
    B = cases.batches()
    e = B["between_160x120"].expect
    assert (e["key_pts"][0, :, 1:] == -1).all() and (e["key_pts"][0, :, 0] >= 0).all()          # features in no quadrant
    e = B["between_33x47"].expect["key_pts"][0]
    assert (e[:, 1] == e[:, 4]).all() and (e[:, 2] == e[:, 3]).all() and (e >= 0).all()         # every feature in two
    for key in cases.CAMERAS:
        e = B[f"ties_{key}"].expect["key_pts"][0]
        assert (e < 50).all() and (e >= 0).all(), key                                           # the smaller rank of each tie
        e = B[f"centre_lines_{key}"].expect["key_pts"]
        assert (e[:, :, 0] == 3).all()                                                          # the first of the two centre pixels
        b = B[f"bad_pixels_{key}"]
        e = b.expect
        bad = np.arange(2, 2 + b.seqs[0].n_bad - 2)                                             # (the last two set a cell)
        ok = np.setdiff1d(np.arange(e["n_points"][0]), bad)
        cell = [chk.cell_of(e["px"][0, 1, r], *b.grid) for r in ok]
        assert sorted(set(cell)) == list(np.flatnonzero(e["occupancy"][0])) and e["occupancy"][0, 0] == 1 and e["occupancy"][0, -1] == 1
        assert all(chk.cell_of(e["px"][0, 1, r], *b.grid) == -1 for r in bad)
        assert e["key_pts"][0, 0, 0] == 0 and np.isnan(e["px"][0, 0, 0]).all()                  # a NaN on rank 0 is never replaced
    e = B["failed_between"].expect
    assert list(e["n_points"]) == [61, 0, 61, 0, 0, 61] and not e["occupancy"][1].any() and (e["key_pts"][1] == -1).all()
    for n in cases.EQUAL_DEPTH_COUNTS:
        b = B[f"equal_depths_{n}"]
        z = np.sort(b.seqs[0].point_w[b.seqs[0].point_ok != 0, 2] + b.seqs[0].T_cur_w[11])
        assert b.expect["depth_mean"][0] == z[n // 2] and b.expect["depth_min"][0] == z[0]
        assert n < 5 or z[n // 2 - 1] == z[n // 2] == z[n // 2 + 1]
    assert {int(s.T_cur_w[0] + s.T_cur_w[4] + s.T_cur_w[8] > 0) for b in B.values() for s in b.seqs} == {0, 1}   # both quaternion branches


def test_identical_sequences_and_repeated_calls_give_the_same_bits(emu):
    for name, twins in (("failed_between", (0, 2, 5)), ("sixteen", (0, 3, 15))):
        b = cases.batches()[name]
        _, one = call_first_map(emu, b)
        _, two = call_first_map(emu, b)
        for k in one.view:
            assert same_bits(one.view[k], two.view[k]), k
            for j in twins[1:]:
                assert same_bits(one.view[k][twins[0]], one.view[k][j]), (k, j)


def test_first_map_limits_and_error_codes(emu):
    b = cases.batches()["n63"]
    cell_size, n_cols, n_rows = b.grid
    for kw in (dict(n_pts=0), dict(n_seq=0)):                       # successful no-ops that touch nothing
        rc, out = call_first_map(emu, b, **kw)
        assert rc == 0 and out.untouched() and out.guards_intact()
    assert call_first_map(emu, b, n_pts=-1)[0] == -1 and call_first_map(emu, b, n_seq=-1)[0] == -1
    assert call_first_map(emu, b, n_pts=1025)[0] == -2
    for grid in ((0, n_cols, n_rows), (-1, n_cols, n_rows), (cell_size, -1, n_rows), (cell_size, n_cols, -1)):
        assert call_first_map(emu, b, grid=grid, cells=n_cols * n_rows)[0] == -1, grid
    for cells in (n_cols * n_rows - 1, n_cols * n_rows + 1, -1):
        assert call_first_map(emu, b, cells=cells)[0] == -1, cells
    for missing in ("cam", "out") + cases.INPUTS:
        rc, out = call_first_map(emu, b, override={missing: None})
        assert rc == -1 and out.untouched(), missing
    for k in capi.FIRST_MAP_OUTPUTS:
        keep = Guarded(cases.out_shapes(len(b.seqs), b.n_pts, n_cols * n_rows))
        o = capi.FirstMapOut(*[None if n == k else keep.ptr(n) for n in capi.FIRST_MAP_OUTPUTS])
        assert call_first_map(emu, b, override={"out": C.byref(o)})[0] == -1 and keep.untouched(), k


@pytest.mark.parametrize("name", cases.SEED_NAMES)
def test_seeds_have_the_checkers_bits(emu, name):
    c, stride, batch_id = cases.seed_cases()[name]
    rc, out = call_seeds(emu, c, stride, batch_id)
    assert rc == 0 and out.guards_intact()
    compare_bits(out.view, c.expect, name)
    n = cases.check_seed_rule(c, out.view)
    assert np.array_equal(n, c.expect["n_seeds"])
    if name.startswith("threshold_"):
        assert ((c.level < 0) & (c.score.astype(np.float64) > c.threshold)).sum() > 100    # empty cells whose score passes the test
    if name == "no_corner":
        assert not n.any()
    if name == "every_corner":
        assert (n == c.n_cells - 1).all()               # (one cell scores exactly the threshold)
    if name == "eight_frames_zero_depth":
        assert np.isinf(out.view["mu"][1, :n[1]]).all() and np.isinf(out.view["sigma2"][1, :n[1]]).all()
    # without the optional columns: the same required ones, the optional ones untouched
    rc, bare = call_seeds(emu, c, stride, batch_id, optional=False)
    assert rc == 0 and bare.guards_intact()
    for k in capi.SEED_INIT_OUTPUTS:
        if k in ("type", "grad"):
            assert (bare.view[k] == 0x55).all() if k == "type" else np.isnan(bare.view[k]).all()
        else:
            assert same_bits(bare.view[k], out.view[k]), k


def test_seed_limits_and_error_codes(emu):
    c, stride, batch_id = cases.seed_cases()["wide_stride"]
    rc, out = call_seeds(emu, c, stride, batch_id, n_frames=0)
    assert rc == 0 and out.untouched()
    rc, out = call_seeds(emu, c, stride, batch_id, n_cells=0)       # no cell: no seed, every record zeroed
    assert rc == 0 and not out.view["n_seeds"].any() and not out.view["mu"].any() and not out.view["px"].any() and out.guards_intact()
    assert call_seeds(emu, c, stride, batch_id, n_frames=-1)[0] == -1 and call_seeds(emu, c, stride, batch_id, n_cells=-1)[0] == -1
    assert call_seeds(emu, c, c.n_cells - 1, batch_id)[0] == -1     # seed_stride < n_cells
    for missing in ("cam", "xy", "level", "score", "frame_index", "depth_mean", "depth_min", "out"):
        rc, out = call_seeds(emu, c, stride, batch_id, override={missing: None})
        assert rc == -1 and out.untouched(), missing
    for k in capi.SEED_INIT_OUTPUTS:
        keep = Guarded(chk.seed_out_shapes(c.n_frames, stride))
        o = capi.SeedInitOut(*[None if n == k else keep.ptr(n) for n in capi.SEED_INIT_OUTPUTS])
        rc = call_seeds(emu, c, stride, batch_id, override={"out": C.byref(o)})[0]
        assert rc == (0 if k in ("type", "grad") else -1), k
    cam = cases.camera(160, 120)
    cam.model = 7
    c2 = cases.make_corners(7, 2, 70, 0.5, cam)
    assert call_seeds(emu, c2, stride, batch_id)[0] == -1
