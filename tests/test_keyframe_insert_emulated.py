"""svo_hip_keyframe_insert (K12, csrc/keyframe_insert.hip) compiled for the CPU through tests/host/hip_emu.h and run as a program
of its own (tests/keyframe_insert_host.py) on the cases of tests/keyframe_insert_cases.py, against the list-based checker
(tests/keyframe_insert_checker.py): EVERY array of the state and EVERY output, byte for byte, after every call -- there is no
floating-point result here, only integers and copies of input doubles.  Each case runs under the emulator's three schedules
(work-items in order, in reverse, wave by wave); every array lies between guard bands and the outputs start poisoned.

Measured on the emulation: all 37 batches have the checker's bytes under the three schedules."""
import numpy as np
import pytest

import keyframe_insert_cases as cases
import keyframe_insert_checker as chk
import keyframe_insert_host as host
from host_buffers import same_bits


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """schedule -> name -> per call (return code, state, outputs): one process per schedule"""
    tmp = str(tmp_path_factory.mktemp("keyframe_insert"))
    return {s: host.run(cases.batches(), s, tmp) for s in host.SCHEDULES}


@pytest.mark.parametrize("schedule", host.SCHEDULES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_keyframe_insert_has_the_checkers_bytes(results, name, schedule):
    host.compare(results[schedule][name], cases.batches()[name], (name, schedule))


def test_argument_errors_touch_nothing():
    import subprocess
    r = subprocess.run([host.program(), "args"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-2000:])


def test_a_sequence_that_is_no_keyframe_or_overflows_keeps_every_byte(results):
    for name in ("results_and_positions", "overflow", "bad_kf_list"):
        b = cases.batches()[name]
        _, state, out = results["inorder"][name][0]
        quiet = [s for s in range(b.B) if b.inputs[0]["result"][s] != cases.IS_KF or out["status"][s] != 0]
        assert quiet, name
        for s in quiet:
            for k in chk.STATE:
                per = lambda a: np.asarray(a).reshape(b.B, -1)[s]
                assert same_bits(per(state[k]), per(b.state[k])), (name, s, k)
            assert (out["kf_new_slot"][s], out["kf_removed_slot"][s], out["n_promoted"][s], out["n_points_deleted"][s]) == (-1, -1, 0, 0)


def test_identical_sequences_give_identical_state_wherever_they_stand(results):
    b = cases.batches()["results_and_positions"]         # sequences 0, 2 and 6 are one sequence; 1, 3 and 7 differ in a result that does not act
    _, state, out = results["waves"]["results_and_positions"][0]
    K = b.dims[0]
    for i, j in ((0, 2), (0, 6), (1, 3), (3, 7)):
        for k in chk.OUTPUTS:
            assert out[k][i] == out[k][j], (k, i, j)
        for k in chk.STATE:
            a = np.asarray(state[k]).reshape(b.B, -1)
            x, y = a[i], a[j]
            if k == "obs_kf":                            # (the frame index carries the sequence: b * K + slot, in the records of the lists)
                live = (np.arange(b.dims[3])[None, :] < np.asarray(state["pt_n_obs"])[i][:, None]).ravel()
                x, y = x[live] - i * K, y[live] - j * K
            assert same_bits(x, y), (k, i, j)


def test_what_the_cases_cover():
    """(the properties the cases are there for, read off the checker's answers)"""
    B = cases.batches()
    out = lambda name, call=0: B[name].expect[call][1]
    assert list(out("removal_none_first_middle_last")["kf_removed_slot"] >= 0) == [False, True, True, True, True]
    b = B["freed_slot_reused"]
    assert out(b.name, 0)["kf_removed_slot"][0] == out(b.name, 1)["kf_new_slot"][0] >= 0 and list(out(b.name, 1)["status"]) == [0, 0, 1]
    assert list(out("overflow")["status"]) == [0, 1, 1, 1, 1, 1, 0] and (out("overflow_fits")["status"] == 0).all()
    assert list(out("bad_kf_list")["status"]) == [2, 2, 2, 0] and (out("bad_kf_remove")["kf_removed_slot"] == -1).all()
    assert (out("bad_kf_remove")["status"] == 0).all()
    assert list(out("candidates_160x120")["n_promoted"]) == [0, 2, 3, 3, 1, 2]
    for key in ("160x120", "47x33", "33x47"):
        K = cases.HAND_DIMS[0]
        kp = lambda name, slot: list(B[f"{name}_{key}"].expect[0][0]["kf_key_pts"][slot])
        before = lambda name, slot: list(B[f"{name}_{key}"].state["kf_key_pts"][slot])
        # an appended feature beats the standing key point only when something triggers the re-scan: the two results differ
        assert kp("kp_appended_no_trigger", 1) == before("kp_appended_no_trigger", 1) and kp("kp_appended_no_trigger", 1)[1] == 1
        assert kp("kp_appended_trigger", 1)[1] == 6 and kp("kp_appended_trigger", 1)[0] != 0
        assert kp("kp_tie_keeps_incumbent", 1)[1] == 6                         # a tie keeps the standing key point
        assert kp("kp_one_after_the_other", 1)[1] == 1                         # re-scanned from NULL: the first of the tie
        new = int(out(f"kp_new_frame_{key}")["kf_new_slot"][0])
        assert kp("kp_new_frame", new)[0] != 0 and B[f"kp_new_frame_{key}"].expect[0][0]["ftr_point"][new, 0] == -1
        assert kp("kp_two_frames", 1)[0] != 0 and kp("kp_two_frames", 2)[0] != 0
        three = B[f"candidates_{key}"].expect[0][0]
        assert list(three["ftr_point"][2 * K + 1, 3:6]) == [21, 22, 20] and list(three["ftr_point"][3 * K + 1, 3:6]) == [20, 21, 22]
    # points with one, two and three records met a leaving keyframe
    b = B["few_records_47x33"]
    n_before = {int(b.state["pt_n_obs"][s, p]) for s in range(b.B) for p in b.state["ftr_point"][s * b.dims[0] + b.state["kf_list"][s, b.inputs[0]["kf_remove"][s]]] if p >= 0}
    assert {1, 2, 3} <= n_before
    rows = B["rows_255_256_257"]
    assert [int(n) for n in rows.expect[0][0]["kf_n_fts"][[int(s) * rows.dims[0] + int(k) for s, k in enumerate(rows.expect[0][1]["kf_new_slot"])]]] == [255, 256, 257, 257]
