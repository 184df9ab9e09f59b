"""How the pose optimizer's wave kernel (csrc/pose_optimizer_wave.hip: one frame, one wave and one block of the dynamic LDS per
workgroup) maps frames to workgroups, without a GPU: the host-emulated library on the batches of tests/pose_wg_map_cases.py --
launches of 1, 2, 3, 4, 5 and 9 frames against the oracle with the requirements of tests/pose_lds_cases.py, then two batches in
which every frame must come out byte for byte as it does alone: nine frames of 200 slots that leave the kernel by every exit,
and the live counts 1 .. 256 of the 256-slot row.  What a frame returns must not depend on the batch it is in."""
import ctypes as C

import numpy as np
import pytest

import pose_lds_cases as cases
import pose_wg_map_cases as wg
from host_buffers import ptr
from oracle import pytrack
from rpg_svo_amd import capi


@pytest.fixture(scope="module")
def emu():
    from emu_build import build_emulated
    return build_emulated(())


@pytest.fixture(scope="module")
def shared(oracle):
    """the scene, the rows and the oracle's answers, computed once for every test of this file"""
    scene = cases.make_scene()
    orc = pytrack.Track("orc")
    rows = {ns: cases.make_row(scene, ns) for ns in wg.ROWS}
    want = {ns: cases.oracle_row(orc, scene, rows[ns]) for ns in wg.ROWS}
    mixed, mixed_want = wg.mixed_batch(orc, scene, rows[200])
    return dict(scene=scene, rows=rows, want=want, mixed=mixed, mixed_want=mixed_want, first={})


def runner(emu, scene, entry="svo_hip_pose_optimize", n_iter=cases.N_ITER):
    cs = capi.camera(scene.cam)

    def run(batch):
        B, ns = len(batch["n"]), batch["ns"]
        T, hp = batch["T0"].copy(), batch["hp"].copy()
        Cov, stats, ran = np.zeros((B, 36)), np.zeros((B, 4)), np.full(B, -1, np.int32)
        rc = getattr(emu, entry)(C.byref(cs), B, ptr(batch["n"]), ns, ptr(batch["f"]), ptr(batch["level"]), ptr(batch["pos"]), ptr(hp),
                                 C.c_double(cases.THRESH), n_iter, ptr(T), ptr(Cov), ptr(stats), ptr(ran), None)
        assert rc == 0, rc
        return T, Cov, stats, ran, hp
    return run


@pytest.mark.parametrize("B", wg.BATCHES)
@pytest.mark.parametrize("ns", wg.ROWS)
def test_emulated_batch_sizes(emu, shared, ns, B):
    row = shared["rows"][ns]
    got = wg.run_in_chunks(runner(emu, shared["scene"]), row, B)
    cases.check(dict(row, T0=row["T0"].reshape(cases.B, 12)), shared["want"][ns], *got)
    first = shared["first"].setdefault(ns, got)  # (B = 1: every frame alone)
    for x, y in zip(first, got):
        assert wg.same_bytes(x, y), (ns, B)


def test_emulated_neighbours_do_not_show(emu, shared):
    scene, batch, want = shared["scene"], shared["mixed"], shared["mixed_want"]
    run, run_deferred = runner(emu, scene), runner(emu, scene, "svo_hip_pose_optimize_deferred")
    got, deferred = run(batch), run_deferred(batch)
    print("frames:", batch["what"], "oracle iterations:", [o["n_iter_done"] for o in want], "ran (deferred):", deferred[3].tolist())
    wg.check_mixed_classes(batch, want, deferred[3])
    wg.check_frames(batch, want, *got)
    assert got[3].tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 1]  # (the handed-over frame finished by the ordered kernel)
    wg.assert_alone_equals_batch(run, batch, got)
    wg.assert_alone_equals_batch(run_deferred, batch, deferred)


def test_emulated_width(emu, shared):
    scene, row = shared["scene"], shared["rows"][256]
    idx = wg.width_frames(row)
    batch = wg.from_row(row, idx)
    run = runner(emu, scene)
    got = run(batch)
    wg.check_frames(batch, [shared["want"][256][i] for i in idx], *got)
    wg.assert_alone_equals_batch(run, batch, got)
