"""The cases of tests/keyframe_insert_cases.py tell the rule of svo_hip_keyframe_insert from its likely mistakes: every named
mutant of the checker (tests/keyframe_insert_checker.py, MUTANTS) must give other bytes than the checker on at least one case.
A case set that lets a mutant through would let a kernel with that mistake through.  No kernel runs here.

  push_back                  addFrameRef appends instead of pushing to the front
  promote_before_frame_ref   addCandidatePointToFrame before the new frame's records exist
  delete_at_one              a point goes with its keyframe at n_obs <= 1 instead of <= 2
  no_rescan                  removeKeyPoint clears the slot and does not run setKeyPoints
  rescan_from_null           the re-scan starts from NULL instead of from the key points still standing
  rescan_on_final_state      the re-scans run after the walk, on the final state, instead of in place
  appended_skipped           the walk of the leaving keyframe stops before the features promoted into it
  remove_before_promote      safeDeleteFrame before addCandidatePointToFrame
  new_frame_at_front         the new keyframe goes to the front of keyframes_"""
import numpy as np
import pytest

import keyframe_insert_cases as cases
import keyframe_insert_checker as chk
from host_buffers import same_bits


def differs(b, mutant):
    cur = b.state
    for inp, (want_state, want_out) in zip(b.inputs, b.expect):
        state, out = chk.insert(b.cam, cur, inp, mutant=mutant)
        if any(not same_bits(out[k], want_out[k]) for k in chk.OUTPUTS) or any(not same_bits(state[k], want_state[k]) for k in chk.STATE):
            return True
        cur = want_state
    return False


@pytest.mark.parametrize("mutant", chk.MUTANTS)
def test_every_mutant_is_caught(mutant):
    caught = [name for name, b in cases.batches().items() if b.well_formed and differs(b, mutant)]
    print(f"{mutant}: caught by {len(caught)} of {len(cases.NAMES)} batches: {caught[:6]}")
    assert caught, mutant


def test_the_checker_is_the_rule_it_is_mutated_from():
    """(no mutant: the stored answers come back, so `differs` compares like with like)"""
    assert not any(differs(b, None) for b in cases.batches().values())


def test_hand_built_cases_catch_the_key_point_mutants_on_their_own():
    """the re-scan rules are pinned by cases a reader can follow, not only by the random maps"""
    B = cases.batches()
    for key in ("160x120", "47x33", "33x47"):
        assert differs(B[f"kp_appended_trigger_{key}"], "no_rescan")
        assert differs(B[f"kp_tie_keeps_incumbent_{key}"], "rescan_from_null")
        assert differs(B[f"kp_one_after_the_other_{key}"], "rescan_on_final_state")
        assert differs(B[f"kp_new_frame_{key}"], "appended_skipped") and differs(B[f"kp_new_frame_{key}"], "remove_before_promote")
        assert differs(B[f"kp_other_keyframe_{key}"], "delete_at_one") and differs(B[f"kp_other_keyframe_{key}"], "push_back")
