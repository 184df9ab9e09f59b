"""Frames per workgroup of the pose optimizer's wave kernel (csrc/pose_optimizer_wave.hip: one frame, one wave and one block of
the dynamic LDS per workgroup) on the GPU, through tracking.optimize_gauss_newton on the batches of tests/pose_wg_map_cases.py:
launches of 1, 2, 3, 4, 5 and 9 frames against the oracle with the requirements of tests/pose_lds_cases.py, then two batches in
which every frame must come out byte for byte as it does alone -- nine frames of 200 slots that leave the kernel by every exit
(n = 0, no flag set, handed over and finished by the ordered kernel, converged after two iterations, all ten iterations, four
ordinary ones), and the live counts 1, 64, 65, 192, 193 and 256 of the 256-slot row."""
import numpy as np
import pytest
import torch

import pose_lds_cases as cases
import pose_wg_map_cases as wg
from oracle import pytrack
from rpg_svo_amd import tracking

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shared(oracle):
    """the scene, the rows and the oracle's answers, computed once for every test of this file"""
    scene = cases.make_scene()
    orc = pytrack.Track("orc")
    rows = {ns: cases.make_row(scene, ns) for ns in wg.ROWS}
    want = {ns: cases.oracle_row(orc, scene, rows[ns]) for ns in wg.ROWS}
    mixed, mixed_want = wg.mixed_batch(orc, scene, rows[200])
    return dict(scene=scene, rows=rows, want=want, mixed=mixed, mixed_want=mixed_want, first={})


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda:0")


def runner(scene, n_iter=cases.N_ITER, **kw):
    def run(batch):
        r = tracking.optimize_gauss_newton(scene.cam, dev(batch["n"], torch.int32), dev(batch["f"], torch.float64),
                                           dev(batch["level"], torch.int32), dev(batch["pos"], torch.float64), dev(batch["hp"], torch.uint8),
                                           dev(batch["T0"], torch.float64), cases.THRESH, n_iter, **kw)
        torch.cuda.synchronize()
        return r.T_f_w.cpu().numpy(), r.Cov.cpu().numpy(), r.stats.cpu().numpy(), r.ran.cpu().numpy(), r.has_point.cpu().numpy()
    return run


@pytest.mark.parametrize("B", wg.BATCHES)
@pytest.mark.parametrize("ns", wg.ROWS)
def test_pose_batch_sizes(gpu_device, shared, ns, B):
    row = shared["rows"][ns]
    got = wg.run_in_chunks(runner(shared["scene"]), row, B)
    cases.check(dict(row, T0=row["T0"].reshape(cases.B, 12)), shared["want"][ns], *got)
    first = shared["first"].setdefault(ns, got)  # (B = 1: every frame alone)
    for x, y in zip(first, got):
        assert wg.same_bytes(x, y), (ns, B)


def test_pose_neighbours_do_not_show(gpu_device, shared):
    scene, batch, want = shared["scene"], shared["mixed"], shared["mixed_want"]
    run, run_deferred = runner(scene), runner(scene, deferred=True)
    got, deferred = run(batch), run_deferred(batch)
    print("frames:", batch["what"], "oracle iterations:", [o["n_iter_done"] for o in want], "ran (deferred):", deferred[3].tolist())
    wg.check_mixed_classes(batch, want, deferred[3])
    wg.check_frames(batch, want, *got)
    assert got[3].tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 1]  # (the handed-over frame finished by the ordered kernel)
    wg.assert_alone_equals_batch(run, batch, got)
    wg.assert_alone_equals_batch(run_deferred, batch, deferred)


def test_pose_width(gpu_device, shared):
    scene, row = shared["scene"], shared["rows"][256]
    idx = wg.width_frames(row)
    batch = wg.from_row(row, idx)
    run = runner(scene)
    got = run(batch)
    wg.check_frames(batch, [shared["want"][256][i] for i in idx], *got)
    wg.assert_alone_equals_batch(run, batch, got)
