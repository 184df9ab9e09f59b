"""The rule of tests/map_mirror_cases.py judged on its own, without a GPU and without the library under test: it passes the
independent walk's own answer on every case, fails on one targeted corruption per output, and rejects each named mutant of the
walk (tests/map_walk_reference.py: MUTANTS, the slips a kernel that orders by keys and fetches records eight at a time could
make) on at least one named case.  The case x mutant table is printed; no mutant survives and no case is idle.  What an emulated
or a device test can pass is therefore what this rule lets through."""
import numpy as np
import pytest

import map_mirror_cases as mc
import map_walk_reference as W

TOL = 1e-9    # the device's bound to the oracle (the walk's own pixels are mpmath's, 1e-13 from the oracle's)


def rejected(c, step, answer):
    try:
        mc.check_answer(c, step, answer, TOL)
    except AssertionError:
        return True
    return False


def test_every_mutant_is_rejected_and_every_case_is_used(oracle):
    names = list(W.MUTANTS)
    killed = {}
    for name, kind in mc.CASES:
        c = mc.case(name, kind)
        for s in c.steps:
            assert not rejected(c, s, mc.wanted(c, s)[0]), (name, s.label)
        for m in names:
            walk = W.MUTANTS[m]()
            killed[name, kind, m] = any(rejected(c, s, walk.walk(s.mp, c.cam, s.first_cell, s.max_cells)) for s in c.steps)
    width = max(len(i) for i in mc.CASE_IDS)
    print("\n" + " " * width + "  " + " ".join(f"{i:2d}" for i in range(len(names))))
    for (name, kind), cid in zip(mc.CASES, mc.CASE_IDS):
        print(f"{cid:{width}s}  " + " ".join(" x" if killed[name, kind, m] else " ." for m in names))
    for i, m in enumerate(names):
        print(f"{i:2d}  {m}")
    survivors = [m for m in names if not any(killed[n, k, m] for n, k in mc.CASES)]
    idle = [n for n in mc.CASE_NAMES if not any(killed[n, "pinhole", m] for m in names)]
    assert not survivors and not idle, (survivors, idle)
    # what each case was built for, it catches
    for n, m in (("records_8_and_9", "first eight records for the close view"), ("many_views", "first eight records for the first meeting"),
                 ("many_views", "non-overlapping keyframes ignored in the close view"), ("behind_camera", "a depth test"),
                 ("close_view_ties", "last record wins a cosine tie"), ("close_view_ties", "cos > 0.5 required"),
                 ("crowded_cell", "equal types in entry order"), ("cuts", "the cut counts cells with visits"), ("cuts", "the cut stops one cell late"),
                 ("key_limits", "first meeting by position regardless of rank")):
        assert killed[n, "pinhole", m], (n, m)


def answer_as_outputs(c, step):
    """the Outputs a correct backend leaves: the walk's answer written into poisoned buffers"""
    w = mc.wanted(c, step)[0]
    out = mc.outputs_for(step)
    V, M = int(w["header"][2]), int(w["header"][3])
    out["d_header"][:] = w["header"]
    out["d_point_cell"][:] = w["point_cell"]
    seen = w["point_cell"] >= -1
    out["d_point_px"][seen] = w["point_px"][seen]
    out["d_kf_count"][:] = w["kf_count"]
    for k in mc.VISIT_KEYS:
        out[k][:V] = w[k[2:]]
    out["d_trial_cur"][:M] = step.mp["cur"]
    out["d_trial_pos"][:M], out["d_trial_px"][:M], out["d_trial_cell"][:M] = w["trial_pos"], w["trial_px"], w["trial_cell"]
    out["d_trial_obs_begin"][:M], out["d_trial_obs_end"][:M] = w["trial_obs"], w["trial_obs"] + 1
    return out, V, M


def test_rule_on_outputs(oracle):
    c = mc.case("capacities")
    step = c.steps[0]
    mc.check_step(c, step, answer_as_outputs(c, step)[0], TOL)
    _, V, M = answer_as_outputs(c, step)
    unseen = int(np.flatnonzero(mc.wanted(c, step)[0]["point_cell"] == -2)[0])
    inside = int(np.flatnonzero(mc.wanted(c, step)[0]["point_cell"] >= 0)[0])

    def fails(change):
        out = answer_as_outputs(c, step)[0]
        change(out)
        with pytest.raises(AssertionError):
            mc.check_step(c, step, out, TOL)

    def put(k, index, value):
        def change(out):
            out[k][index] = value(out[k][index]) if callable(value) else value
        return change

    for k in ("d_point_cell", "d_kf_count", "d_visit_point", "d_visit_cell", "d_visit_trial", "d_trial_obs_begin", "d_trial_obs_end", "d_trial_cell",
              "d_trial_cur"):
        fails(put(k, 0, lambda v: v + 1))
    for i in range(8):
        fails(put("d_header", i, lambda v: v + 1))
    fails(put("d_trial_pos", (M - 1, 2), lambda v: np.nextafter(v, 9.0)))                 # bit for bit
    fails(put("d_point_px", (inside, 0), lambda v: v + 2e-9))
    fails(put("d_trial_px", (0, 1), lambda v: v + 2e-10))                                 # inside the oracle's bound, outside the walk's
    fails(put("d_point_px", (unseen, 0), 1.0))                                            # written where the point was not projected
    fails(put("d_visit_point", V - 1, mc.POISON))                                         # a visit the entry did not write
    mc.check_step(c, step, answer_as_outputs(c, step)[0], TOL)

    def guard(out):
        out.raw["d_trial_cell"][-1] = 0
    fails(guard)
    # one slot short: nothing written, V = M = 0, end_cell = first_cell
    short = c.steps[1]
    out = mc.outputs_for(short)
    w = mc.wanted(c, short)[0]
    out["d_header"][:5] = 1, w["header"][1], 0, 0, short.first_cell
    out["d_point_cell"][:] = w["point_cell"]
    seen = w["point_cell"] >= -1
    out["d_point_px"][seen] = w["point_px"][seen]
    out["d_kf_count"][:] = w["kf_count"]
    mc.check_step(c, short, out, TOL)
    out["d_visit_cell"][3] = 0
    with pytest.raises(AssertionError):
        mc.check_step(c, short, out, TOL)
    with pytest.raises(AssertionError):                                                   # a backend that ignored the capacity
        mc.check_step(c, short, answer_as_outputs(c, step)[0], TOL)
