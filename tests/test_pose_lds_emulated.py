"""The wave kernel of the pose optimizer (csrc/pose_optimizer_wave.hip: live observations compacted into the wave's LDS block,
a runtime loop over trips of 64) without a GPU: svo_hip_pose_optimize, its deferred entry and the n_iter = 0 hand-over of the
host-emulated library (tests/emu_build.py, default build) on the table of tests/pose_lds_cases.py, against the oracle's
pose_optimizer::optimizeGaussNewton with the requirements of tests/test_tracking_gpu.py::test_pose_optimize."""
import ctypes as C

import numpy as np
import pytest

import pose_lds_cases as cases
from host_buffers import ptr
from oracle import pytrack
from rpg_svo_amd import capi


@pytest.fixture(scope="module")
def emu():
    from emu_build import build_emulated
    return build_emulated(())


@pytest.fixture(scope="module")
def scene():
    return cases.make_scene()


def run(emu, scene, row, n_iter, entry="svo_hip_pose_optimize"):
    B, ns = cases.B, row["ns"]
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
    n, f, level, pos = c(row["n"], np.int32), c(np.tile(row["f"], (B, 1, 1)), np.float64), c(np.tile(row["level"], (B, 1)), np.int32), \
        c(np.tile(row["pos"], (B, 1, 1)), np.float64)
    T, hp = row["T0"].copy(), row["hp"].copy()
    Cov, stats, ran = np.zeros((B, 36)), np.zeros((B, 4)), np.full(B, -1, np.int32)
    cs = capi.camera(scene.cam)
    rc = getattr(emu, entry)(C.byref(cs), B, ptr(n), ns, ptr(f), ptr(level), ptr(pos), ptr(hp), C.c_double(cases.THRESH), n_iter, ptr(T),
                             ptr(Cov), ptr(stats), ptr(ran), None)
    assert rc == 0, rc
    return T, Cov, stats, ran, hp


@pytest.mark.parametrize("ns", cases.ROWS)
def test_emulated_pose_lds_row(emu, oracle, scene, ns):
    row = cases.make_row(scene, ns)
    want = cases.oracle_row(pytrack.Track("orc"), scene, row)
    T, Cov, stats, ran, hp = run(emu, scene, row, cases.N_ITER)
    devs = cases.check(row, want, T, Cov, stats, ran, hp)
    print(f"n_stride {ns}: pose against the oracle, frames of >= 20 live observations: max {max(devs, default=0):.3e} "
          f"median {np.median(devs) if devs else 0:.3e}")
    if ns >= 64:  # (7 slots: the only wrong point is slot 0, which never moves)
        assert cases.moved_and_pruned(row, want), "no frame of this row prunes an observation that compaction moved"

    # the deferred entry: the same bits on the frames the wave kernel takes, the others untouched with ran == 2
    Td, _, _, rand, hpd = run(emu, scene, row, cases.N_ITER, "svo_hip_pose_optimize_deferred")
    assert not (ran == 2).any()
    taken = rand != 2
    assert np.array_equal(Td[taken], T[taken]) and np.array_equal(rand[taken], ran[taken]) and np.array_equal(hpd[taken], hp[taken])
    assert np.array_equal(Td[~taken], row["T0"][~taken]) and np.array_equal(hpd[~taken], row["hp"][~taken])
    live = np.array([row["hp"][b, :row["n"][b]].sum() for b in range(cases.B)])
    assert taken.any() and taken[live == 0].all()  # (a frame without an observation returns at once: ran == 0)

    # n_iter = 0: every frame with an observation is handed over, and the ordered kernel finishes it
    T0f, _, st0f, ran0f, hp0f = run(emu, scene, row, 0)
    T0d, _, _, ran0d, hp0d = run(emu, scene, row, 0, "svo_hip_pose_optimize_deferred")
    T0o, _, st0o, ran0o, hp0o = run(emu, scene, row, 0, "svo_hip_pose_optimize_ordered")
    assert np.array_equal(ran0d, np.where(live > 0, 2, 0)) and np.array_equal(T0d, row["T0"]) and np.array_equal(hp0d, row["hp"])
    assert np.array_equal(T0f, T0o) and np.array_equal(ran0f, ran0o) and np.array_equal(hp0f, hp0o) and np.array_equal(st0f, st0o)
