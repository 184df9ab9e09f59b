"""Row N2 without a GPU, at the edges: the named cases of tests/map_mirror_cases.py -- more than eight observation records, more
than 1024 cells, a crowded cell, points behind the camera, the key ranges and the 4096-point limit at their last values, exact
borders, cosine ties, cuts, capacities, a patch that moves first meetings -- through the host-emulated svo_hip_reproject_map
(tests/emu_build.py, tests/map_mirror_host.py) under the one rule of that module: integers identical to the independent walk of
tests/map_walk_reference.py and to the oracle, pixels to 1e-12 of the oracle (the bound of tests/test_map_mirror_emulated.py),
outputs poisoned and guarded.  Then the entry's argument checks, row by row."""
import pytest

import map_mirror_cases as mc
import map_mirror_host as mh

PX_TOL_ORACLE = 1e-12


@pytest.fixture(scope="module")
def emu():
    from emu_build import build_emulated
    return build_emulated(())


@pytest.mark.parametrize("name,kind", mc.CASES, ids=mc.CASE_IDS)
def test_emulated_edges(emu, oracle, name, kind):
    c = mc.case(name, kind)
    d_oracle, d_walk = mc.check_case(c, mh.run_case(emu, c), PX_TOL_ORACLE)
    print(f"{name}-{kind}: largest px difference {d_oracle:.3g} to the oracle, {d_walk:.3g} to the mpmath walk")


def test_emulated_argument_table(emu, oracle):
    mc.check_arguments(emu, lambda cam, step: mh.make_call(emu, cam, step)[:2], PX_TOL_ORACLE)
