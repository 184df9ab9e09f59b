"""svo_hip_pose_optimize_into, the `ran` scan of the fix-up launch and the wave kernel's compaction without a GPU: the cases of
tests/pose_into_cases.py on the host-emulated library (tests/emu_build.py, default build).  The new entry against copy + the old
entry byte for byte (poisoned outputs between guard bands, inputs unchanged, in == out) on the nine frames of
pose_wg_map_cases.mixed_batch in batches of 1, 8 and 200, on rows of 64, 200, 250, 256 and 257 slots and with n_iter = 0; the
fix-up launch with the handed-over frame at every place of a 64-chunk that matters; rows whose live slots sit in particular trips
against the oracle."""
import numpy as np
import pytest

import pose_into_cases as into
import pose_lds_cases as cases
import pose_wg_map_cases as wg
from oracle import pytrack


class Host:
    """the backend of pose_into_cases on host memory"""

    def __init__(self, lib):
        self.lib = lib

    def up(self, a):
        return np.array(a, copy=True, order="C")

    def down(self, buf, dtype, count, offset=0):
        return np.frombuffer(buf.tobytes(), dtype=dtype, count=count, offset=offset).copy()

    def addr(self, buf):
        return buf.ctypes.data

    def sync(self):
        pass


@pytest.fixture(scope="module")
def be():
    from emu_build import build_emulated
    return Host(build_emulated((), bind=into.ENTRIES))


@pytest.fixture(scope="module")
def shared(oracle):
    scene = cases.make_scene()
    orc = pytrack.Track("orc")
    mixed, mixed_want = wg.mixed_batch(orc, scene, cases.make_row(scene, 200))
    return dict(scene=scene, orc=orc, mixed=mixed, mixed_want=mixed_want)


@pytest.mark.parametrize("B", into.BATCH_SIZES)
def test_emulated_into_every_exit(be, shared, B):
    """n = 0, no flag set, handed over and finished, exact projection, all ten iterations, short n, 20 % dead"""
    scene, mixed = shared["scene"], shared["mixed"]
    if B == 1:
        for b in range(len(mixed["n"])):
            into.check_into(be, scene.cam, wg.take(mixed, [b]), what=mixed["what"][b])
        return
    batch = into.stretch(mixed, B)
    got = into.check_into(be, scene.cam, batch, what=B)
    m = min(B, len(mixed["n"]))
    wg.check_frames(wg.take(batch, range(m)), shared["mixed_want"][:m], *[x[:m] for x in got])
    assert got[3][:m].tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 1][:m]


@pytest.mark.parametrize("ns", into.ROWS)
def test_emulated_into_rows(be, shared, ns):
    scene = shared["scene"]
    row = cases.make_row(scene, ns)
    batch = wg.from_row(row, range(cases.B))
    got = into.check_into(be, scene.cam, batch, what=ns)
    cases.check(dict(row, T0=row["T0"].reshape(cases.B, 12)), cases.oracle_row(shared["orc"], scene, row), *got)


@pytest.mark.parametrize("ns", (200, 257))
def test_emulated_into_without_an_iteration(be, shared, ns):
    """n_iter = 0: every frame with an observation is handed over, and the scan runs all of a chunk's frames one after the other"""
    scene = shared["scene"]
    batch = shared["mixed"] if ns == 200 else wg.from_row(cases.make_row(scene, ns), range(cases.B))
    got = into.check_into(be, scene.cam, batch, 0, what=ns)
    into.assert_same(got, into.call_in_place(be, scene.cam, batch, 0, "svo_hip_pose_optimize_ordered"), "ordered")
    live = np.array([batch["hp"][b, :max(batch["n"][b], 0)].sum() for b in range(len(batch["n"]))])
    assert got[3].tolist() == (live > 0).astype(int).tolist()


@pytest.mark.parametrize("case", list(into.SCAN_CASES))
def test_emulated_fixup_scan(be, shared, case):
    B, flagged = into.SCAN_CASES[case]
    into.check_scan(be, shared["scene"].cam, into.scan_batch(shared["scene"], B, flagged), flagged)


def test_emulated_live_slots_by_trip(be, shared):
    scene = shared["scene"]
    batch = into.layout_batch(scene)
    got = into.check_into(be, scene.cam, batch, what="layout")
    wg.check_frames(batch, wg.oracle_batch(shared["orc"], scene, batch), *got)
    wg.assert_alone_equals_batch(lambda one: into.call_in_place(be, scene.cam, one), batch, got)
