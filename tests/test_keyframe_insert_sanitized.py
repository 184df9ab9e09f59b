"""K12's memory accesses and arithmetic under AddressSanitizer and UndefinedBehaviorSanitizer, without a GPU and without
loading anything into Python: the sources of tests/keyframe_insert_host.py built with -fsanitize=address,undefined
(tests/emu_build.py's build_program) into a program of its own, which runs the host-emulated svo_hip_keyframe_insert on heap
blocks of exactly the documented sizes.  It must exit 0 with no report, and its results must still be the checker's bytes.

  limits     257 and 1024 rows, K = 64 with 63 and 64 keyframes, R = 64 with points seen by up to 63 keyframes, n beyond n_stride
  overflow   every capacity exceeded, next to sequences that fit
  bad        every index that cannot index: points, records, key points, kf_remove, kf_list, counts beyond their capacity"""
import pytest

import keyframe_insert_cases as cases
import keyframe_insert_host as host


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("keyframe_insert_asan"))


def test_the_limit_shapes_stay_inside_their_buffers(tmp):
    batches = cases.limit_batches()
    got = host.run(batches, "inorder", tmp, sanitize=True)
    for name, b in batches.items():
        host.compare(got[name], b, name)
    status = batches["limit_1024_rows"].expect[0][1]["status"]
    assert list(status) == [0, 1, 0]                                     # 63 keyframes fit, 64 leave no slot


def test_overflows_and_indices_that_cannot_index_stay_inside_their_buffers(tmp):
    names = ("overflow", "overflow_fits", "bad_indices", "bad_kf_remove", "bad_kf_list", "rows_255_256_257", "freed_slot_reused")
    batches = {n: cases.batches()[n] for n in names}
    for schedule in ("reverse", "waves"):
        got = host.run(batches, schedule, tmp, sanitize=True)
        for name, b in batches.items():
            host.compare(got[name], b, (name, schedule))


def test_argument_errors_under_the_sanitizers():
    from emu_build import run_program
    run_program(host.program(sanitize=True), "args")
