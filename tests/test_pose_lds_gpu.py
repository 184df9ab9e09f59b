"""The table of tests/pose_lds_cases.py on the GPU: the wave kernel of the pose optimizer (live observations compacted into
LDS, a runtime loop over trips of 64) through tracking.optimize_gauss_newton -- sixteen frames per row length, live counts on
every trip boundary, the flag patterns that move observations -- against the oracle and, where present, the reference's own
translation unit, with the requirements of tests/test_tracking_gpu.py::test_pose_optimize; then the deferred entry and the
n_iter = 0 hand-over on the same rows."""
import numpy as np
import pytest
import torch

import pose_lds_cases as cases
from oracle import pytrack
from rpg_svo_amd import tracking

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc(oracle, checker):
    return pytrack.Track(checker)


@pytest.fixture(scope="module")
def scene():
    return cases.make_scene()


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda:0")


def run(scene, row, n_iter, **kw):
    B = cases.B
    r = tracking.optimize_gauss_newton(scene.cam, dev(row["n"], torch.int32), dev(np.tile(row["f"], (B, 1, 1)), torch.float64),
                                       dev(np.tile(row["level"], (B, 1)), torch.int32), dev(np.tile(row["pos"], (B, 1, 1)), torch.float64),
                                       dev(row["hp"], torch.uint8), dev(row["T0"], torch.float64), cases.THRESH, n_iter, **kw)
    torch.cuda.synchronize()
    return r.T_f_w.cpu().numpy(), r.Cov.cpu().numpy(), r.stats.cpu().numpy(), r.ran.cpu().numpy(), r.has_point.cpu().numpy()


@pytest.mark.parametrize("ns", cases.ROWS)
def test_pose_lds_row(gpu_device, orc, scene, ns):
    row = cases.make_row(scene, ns)
    want = cases.oracle_row(orc, scene, row)
    T, Cov, stats, ran, hp = run(scene, row, cases.N_ITER)
    devs = cases.check(row, want, T, Cov, stats, ran, hp)
    print(f"n_stride {ns}: pose against the oracle, frames of >= 20 live observations: max {max(devs, default=0):.3e} "
          f"median {np.median(devs) if devs else 0:.3e}")
    if ns >= 64:  # (7 slots: the only wrong point is slot 0, which never moves)
        assert cases.moved_and_pruned(row, want), "no frame of this row prunes an observation that compaction moved"

    # the deferred entry: the same bits on the frames the wave kernel takes, the others untouched with ran == 2
    Td, _, _, rand, hpd = run(scene, row, cases.N_ITER, deferred=True)
    assert not (ran == 2).any()
    taken = rand != 2
    assert np.array_equal(Td[taken], T[taken]) and np.array_equal(rand[taken], ran[taken]) and np.array_equal(hpd[taken], hp[taken])
    assert np.array_equal(Td[~taken], row["T0"][~taken]) and np.array_equal(hpd[~taken], row["hp"][~taken])
    live = np.array([row["hp"][b, :row["n"][b]].sum() for b in range(cases.B)])
    assert taken.any() and taken[live == 0].all()  # (a frame without an observation returns at once: ran == 0)

    # n_iter = 0: every frame with an observation is handed over, and the ordered kernel finishes it
    T0f, _, st0f, ran0f, hp0f = run(scene, row, 0)
    T0d, _, _, ran0d, hp0d = run(scene, row, 0, deferred=True)
    T0o, _, st0o, ran0o, hp0o = run(scene, row, 0, ordered=True)
    assert np.array_equal(ran0d, np.where(live > 0, 2, 0)) and np.array_equal(T0d, row["T0"]) and np.array_equal(hp0d, row["hp"])
    assert np.array_equal(T0f, T0o) and np.array_equal(ran0f, ran0o) and np.array_equal(hp0f, hp0o) and np.array_equal(st0f, st0o)
