"""The map mirror's memory accesses at its limits under AddressSanitizer and UndefinedBehaviorSanitizer, without a GPU and without
loading anything into Python: tests/host/map_mirror_asan_main.cpp is a program of its own that runs the limit cases of
tests/map_mirror_cases.py (crowded_cell, in_frame_limit, cell_limit, key_limits: the LDS arrays s_bkey / s_bidx / s_sidx /
s_srank[4096] and s_cnt / s_base[2048], the 16-bit entry and cell numbers, all at their last elements) through the host-emulated
svo_hip_reproject_map on heap buffers of exactly the documented sizes.  It must exit 0 with no report, and what it computed is
held against the independent walk and the oracle under the one rule, like the emulated library's results."""
import map_mirror_cases as mc
from emu_build import build_program, run_program


def test_map_mirror_stays_inside_its_buffers_at_the_limits(oracle, tmp_path):
    exe = build_program("map_mirror_asan", ("emu_tu_common.cpp", "emu_tu_map_mirror.cpp", "map_mirror_asan_main.cpp"), deps=(mc.__file__,))
    cases = [mc.case(n) for n in mc.SANITIZED]
    items = [(c.cam, s) for c in cases for s in c.steps]
    mc.write_steps(tmp_path / "in.bin", items)
    run_program(exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"))
    outs = iter(mc.read_outputs(tmp_path / "out.bin", items))
    for c in cases:
        d_oracle, d_walk = mc.check_case(c, [next(outs) for _ in c.steps], 1e-12)
        print(f"{c.name}: largest px difference {d_oracle:.3g} to the oracle, {d_walk:.3g} to the mpmath walk")
