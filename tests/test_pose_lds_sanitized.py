"""The pose optimizer's memory accesses and arithmetic under AddressSanitizer and UndefinedBehaviorSanitizer, without a GPU
and without loading anything into Python: tests/host/pose_lds_asan_main.cpp is a program of its own that runs the table of
tests/pose_lds_cases.py through the host-emulated svo_hip_pose_optimize and svo_hip_pose_optimize_deferred (n_iter = 0) (the wave kernel
with its observations compacted into LDS, the ordered kernel behind it) on heap buffers of exactly the documented sizes and
on dynamic LDS of exactly each launch's byte count.  It must exit 0 with no report, and what it computed is held against the
oracle like the emulated library's results."""
import numpy as np

import pose_lds_cases as cases
from emu_build import build_program, run_program
from oracle import pytrack


def test_pose_optimizer_stays_inside_its_buffers_and_its_lds(oracle, tmp_path):
    # (both kernels of the emulated pose optimizer, with exactly sized dynamic LDS: tests/host/pose_lds_asan_lds.h)
    exe = build_program("pose_lds_asan", ("emu_tu_common.cpp", "pose_lds_asan_tu_wave.cpp", "pose_lds_asan_tu_ordered.cpp", "pose_lds_asan_main.cpp"),
                        deps=("pose_lds_asan_lds.h", cases.__file__))
    scene = cases.make_scene()
    rows = [cases.make_row(scene, ns) for ns in cases.ROWS]
    cases.write_rows(tmp_path / "in.bin", scene, rows)
    run_program(exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"))
    orc = pytrack.Track("orc")
    for row, legs in zip(rows, cases.read_results(tmp_path / "out.bin", rows)):
        cases.check(row, cases.oracle_row(orc, scene, row), *legs[0])
        live = np.array([row["hp"][b, :row["n"][b]].sum() for b in range(cases.B)])
        Td, _, _, rand, hpd = legs[1]  # n_iter = 0, deferred: every frame with an observation handed over untouched
        assert np.array_equal(rand, np.where(live > 0, 2, 0)) and np.array_equal(Td, row["T0"]) and np.array_equal(hpd, row["hp"])
