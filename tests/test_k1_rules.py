"""The rule of tests/k1_cases.py judged on its own, without a GPU and without the library under test: verify() passes under
every profile when it is fed the checker's own answer to a small case (two QVGA frames of 200 and 256 patches) and fails on one
targeted corruption per output.  What an emulated or a device K1 test can pass is therefore what this rule lets through."""
import numpy as np
import pytest

import k1_cases as k1
from rpg_svo_amd import se3

NAME = "counts_256"


@pytest.fixture(scope="module")
def truth(oracle):
    """(case, T_o, res_o, the checker's answer as a K1Answer)"""
    c = k1.case(NAME)
    T_o, res_o = k1.reference(oracle, NAME, c.schedules[0])
    arr = lambda key, dt=None: np.array([np.asarray(r[key]).ravel() if key == "H" else r[key] for r in res_o], dtype=dt)
    return c, T_o, res_o, k1.K1Answer(T_o.copy(), arr("iters"), arr("n_tracked"), arr("stop"), arr("H"), arr("chi2"))


def changed(answer, field, index, value):
    """a copy of `answer` with answer.field[index] = value (a function of the old value, or a value)"""
    a = np.array(getattr(answer, field), copy=True)
    a[index] = value(a[index]) if callable(value) else value
    return answer._replace(**{field: a})


def moved(answer, frame, by):
    """the pose of `frame` moved by an SE(3) log-norm of `by`"""
    xi = np.zeros((1, 6))
    xi[0, 0] = by
    return changed(answer, "pose", frame, se3.mul(se3.exp(xi), answer.pose[frame:frame + 1])[0])


def fails(*args, **kw):
    with pytest.raises(AssertionError):
        k1.verify(*args, **kw)


@pytest.mark.parametrize("profile", list(k1.PROFILES))
def test_the_checkers_own_answer_passes(truth, profile):
    c, T_o, res_o, answer = truth
    m = k1.verify(c, answer, T_o, res_o, k1.PROFILES[profile])
    assert m.d.max() < 1e-14 and m.same.all() and m.H_off == 0.0 and m.chi2_off == 0.0


@pytest.mark.parametrize("profile", list(k1.PROFILES))
def test_poses(truth, profile):
    c, T_o, res_o, answer = truth
    bounds = k1.PROFILES[profile]
    fails(c, moved(answer, 1, 2 * bounds.max_d), T_o, res_o, bounds)
    m = k1.verify(c, moved(answer, 1, 0.5 * bounds.max_d), T_o, res_o, bounds.but(median_d=None))
    assert m.d[0] < 1e-14 and abs(m.d[1] / (0.5 * bounds.max_d) - 1) < 1e-6       # (the rule hands back what it measured)
    fails(c, changed(answer, "pose", (0, 4), np.nan), T_o, res_o, bounds)
    if bounds.median_d is not None:   # one of the two frames past the median bound, inside the maximum: the median is 1.5 x its bound
        assert 3 * bounds.median_d < bounds.max_d
        fails(c, moved(answer, 0, 3 * bounds.median_d), T_o, res_o, bounds)
        k1.verify(c, moved(answer, 0, 3 * bounds.median_d), T_o, res_o, bounds.but(median_d=None))


def test_iteration_sequences(truth):
    c, T_o, res_o, answer = truth
    one = changed(answer, "iters", (0, 1), lambda v: v + 1)
    two = changed(one, "iters", (1, 0), lambda v: v - 1)
    for bounds in (k1.DEVICE, k1.DEVICE_WAVE, k1.EMULATED, k1.EMULATED_BASE, k1.EMULATED_WAVE):
        assert bounds.max_other_seq == 1
        m = k1.verify(c, one, T_o, res_o, bounds)        # one frame of a small batch may part
        assert m.same.tolist() == [False, True]
        fails(c, two, T_o, res_o, bounds)
    fails(c, one, T_o, res_o, k1.SINGLE_STEP)            # (none where the schedule is one step)
    assert k1.DEVICE_SAMPLE.min_same_share == 0.97
    fails(c, one, T_o, res_o, k1.DEVICE_SAMPLE)          # half of the frames is below 97 %
    k1.verify(c, one, T_o, res_o, k1.DEVICE_SAMPLE.but(min_same_share=0.5))


def test_tracked_counts_and_status(truth):
    c, T_o, res_o, answer = truth
    for bounds in k1.PROFILES.values():
        for by in (1, -1):
            fails(c, changed(answer, "n_tracked", 1, lambda v: v + by), T_o, res_o, bounds)
    # a frame with another iteration sequence: its count is compared where the profile says "all" only
    other = changed(changed(answer, "iters", (1, 0), lambda v: v + 1), "n_tracked", 1, lambda v: v - 1)
    k1.verify(c, other, T_o, res_o, k1.DEVICE)
    fails(c, other, T_o, res_o, k1.EMULATED)
    for bounds in (k1.DEVICE, k1.DEVICE_WAVE, k1.DEVICE_SAMPLE, k1.EMULATED_WAVE):
        assert bounds.status
        fails(c, changed(answer, "status", 0, lambda v: 1 - v), T_o, res_o, bounds)


@pytest.mark.parametrize("profile", list(k1.PROFILES))
def test_H_and_chi2(truth, profile):
    """the largest entry of H may be off by rtol + the atol share of itself: three times that fails, a third of it passes"""
    c, T_o, res_o, answer = truth
    bounds = k1.PROFILES[profile]
    frame = 1
    k = int(np.abs(answer.H).argmax() % 36) if np.abs(answer.H).argmax() // 36 == frame else int(np.abs(answer.H[frame]).argmax())
    allowed = bounds.H[0] + bounds.H[1] * np.abs(answer.H).max() / np.abs(answer.H[frame, k])
    fails(c, changed(answer, "H", (frame, k), lambda v: v * (1 + 3 * allowed)), T_o, res_o, bounds)
    m = k1.verify(c, changed(answer, "H", (frame, k), lambda v: v * (1 + allowed / 3)), T_o, res_o, bounds)
    assert m.H_off > 0
    if bounds.chi2 is not None:
        assert bounds.chi2 == 1e-4
        fails(c, changed(answer, "chi2", 0, lambda v: v * (1 + 2e-4)), T_o, res_o, bounds)
        k1.verify(c, changed(answer, "chi2", 0, lambda v: v * (1 + 5e-5)), T_o, res_o, bounds)


def test_unposed_frames(truth):
    """a frame the case lists as unposed: any finite pose, any iteration sequence, no more patches tracked than it has"""
    c, T_o, res_o, answer = truth
    unposed = k1.Case(NAME, c.built, unposed=(0,))
    wild = changed(changed(moved(answer, 0, 0.3), "iters", (0, 0), 7), "n_tracked", 0, int(c.batch.n[0]))
    for bounds in k1.PROFILES.values():
        fails(c, wild, T_o, res_o, bounds)
        k1.verify(unposed, wild, T_o, res_o, bounds)
        fails(unposed, changed(wild, "n_tracked", 0, int(c.batch.n[0]) + 1), T_o, res_o, bounds)
        fails(unposed, changed(wild, "pose", (0, 11), np.inf), T_o, res_o, bounds)
