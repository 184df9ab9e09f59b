"""Row N2, CPU: the C restatement of Reprojector::reprojectMap (oracle/svo_oracle_track.c: orc_reproject_map) against
a literal Python walk of the reference's loops (svo/src/reprojector.cpp:64-142, 151-153, 206-217) over the same
plain-array map -- keyframes closest first, every Feature of a keyframe in list order, "project a point only once",
candidates afterwards in list order, push_back into grid cells, a stable sort per cell -- plus the properties the
batched drop-in relies on (one cell per point, cells in visiting order, the first-batch cut).  The literal walk is
map_walk_reference.literal_walk, here through the oracle's own reproject_point; the same oracle answers are then held, whole --
header, trial_obs and visit_trial included -- against the independent walk of that module, which takes its projections from
mpmath and has the close-view step and the cut."""
import numpy as np
import pytest

from helpers import camera_models, oracle_reproject_map, random_map
from map_walk_reference import REF_WALK, literal_walk
from oracle import pytrack

WHOLE = ("header", "point_cell", "kf_count", "visit_point", "visit_cell", "visit_trial", "trial_obs", "trial_cell", "trial_pos")


@pytest.mark.parametrize("kind", ["pinhole", "atan"])
def test_oracle_restatement_is_the_literal_walk(oracle, kind):
    cam = camera_models()[kind]
    orc = pytrack.Track("orc")
    for seed in range(3):
        mp = random_map(cam, n_kfs=8, n_points=250, n_candidates=200, seed=seed, n_overlap=5)
        r = oracle_reproject_map(mp, cam)
        T_cur = mp["T"][mp["cur"]]
        point_cell, kf_count, visit = literal_walk(mp, lambda p: orc.reproject_point(cam, T_cur, mp["pos"][p], mp["cell_size"], mp["n_cols"])[0])
        assert np.array_equal(r["point_cell"], point_cell)
        assert np.array_equal(r["kf_count"], kf_count)
        assert [(int(p), int(c)) for p, c in zip(r["visit_point"], r["visit_cell"])] == visit
        assert r["header"][1] == (point_cell >= 0).sum() == len(visit) and r["header"][4] == mp["n_cols"] * mp["n_rows"]
        # a trial is a visit with a close view; its observation is one of the point's
        t = r["visit_trial"]
        assert np.array_equal(t[t >= 0], np.arange((t >= 0).sum()))
        for v in np.nonzero(t >= 0)[0]:
            p, o = r["visit_point"][v], r["trial_obs"][t[v]]
            assert mp["obs_begin"][p] <= o < mp["obs_begin"][p] + mp["obs_count"][p]
            assert r["trial_cell"][t[v]] == r["visit_cell"][v] and np.array_equal(r["trial_pos"][t[v]], mp["pos"][p])
        assert (t >= 0).sum() > 20 and (t < 0).sum() > 0   # both kinds occur
        w = REF_WALK.walk(mp, cam)
        for k in WHOLE:
            assert np.array_equal(r[k], w[k]), k
        seen = w["point_cell"] >= -1
        assert np.abs(r["point_px"][seen] - w["point_px"][seen]).max() <= 1e-10 and np.abs(r["trial_px"] - w["trial_px"]).max() <= 1e-10


def test_first_batch_cut_and_continuation(oracle):
    """Cells are taken until max_cells_with_trials of them hold a trial; a second call from end_cell continues the walk:
    together they are the uncut walk (the drop-in's two batches)."""
    cam = camera_models()["pinhole"]
    mp = random_map(cam, seed=7)
    full = oracle_reproject_map(mp, cam)
    a = oracle_reproject_map(mp, cam, 0, 40)
    end = int(a["header"][4])
    cells_with_trials = len(set(a["trial_cell"].tolist()))
    assert cells_with_trials == 40 and a["trial_cell"].max() == end - 1      # the walk stops right after the 40th such cell
    b = oracle_reproject_map(mp, cam, end, 1 << 30)
    assert np.array_equal(np.concatenate([a["visit_point"], b["visit_point"]]), full["visit_point"])
    assert np.array_equal(np.concatenate([a["trial_obs"], b["trial_obs"]]), full["trial_obs"])
    assert np.array_equal(np.concatenate([a["visit_trial"], np.where(b["visit_trial"] >= 0, b["visit_trial"] + a["header"][3], -1)]),
                          full["visit_trial"])
    z = oracle_reproject_map(mp, cam, 0, 0)
    assert z["header"][2] == 0 and z["header"][3] == 0 and z["header"][4] == 0
    for first_cell, max_cells in ((0, 40), (end, 1 << 30), (0, 0), (17, 3)):   # the cut and the start, against the independent walk
        r, w = oracle_reproject_map(mp, cam, first_cell, max_cells), REF_WALK.walk(mp, cam, first_cell, max_cells)
        for k in WHOLE:
            assert np.array_equal(r[k], w[k]), (first_cell, max_cells, k)
