"""TEST INFRASTRUCTURE, not a test.  Batches for tests/test_pose_wg_map_emulated.py and tests/test_pose_wg_map_gpu.py: how the
wave kernel of the pose optimizer (csrc/pose_optimizer_wave.hip) maps frames to workgroups -- PW_WAVES frames per workgroup (one
since profiles/r08a_k4_one_frame_per_workgroup.txt, four before), one wave and one block of the dynamic LDS each -- must not
show in any frame's result.

  * the rows of tests/pose_lds_cases.py (sixteen frames, every live count on a trip boundary) cut into launches of B = 1, 2, 3,
    4, 5 and 9 frames (chunks): a first, a last and a ragged last workgroup whether a workgroup holds 1, 2 or 4 frames;
  * mixed_batch: nine frames of 200 slots that leave the kernel by every exit, next to each other -- n = 0; every flag clear; one
    live observation (singular normal equations: handed over, ran = 2, and finished by the ordered kernel); observations at the
    exact projection (two iterations); gross outliers chosen so that all ten iterations run; four ordinary frames of the row;
  * width_batch: the frames of the 256-slot row with 1, 64, 65, 192, 193 and 256 live observations in one batch: a last trip of
    one lane and of all lanes, and the largest LDS block.

A batch is a dict of per-frame arrays: ns, n [B], f [B,ns,3], level [B,ns], pos [B,ns,3], hp [B,ns], T0 [B,12], what [B]."""
import numpy as np

import pose_lds_cases as cases
from helpers import fuzz_rng
from rpg_svo_amd import se3, synth
from tracking_cases import check_pose

ROWS = (8, 200, 256)
BATCHES = (1, 2, 3, 4, 5, 9)
WIDTH_COUNTS = (1, 64, 65, 192, 193, 256)
MIXED_RAN_DEFERRED = (0, 0, 2, 1, 1, 1, 1, 1, 1)  # what the wave kernel alone leaves in `ran` for the nine frames of mixed_batch


def from_row(row, idx):
    """the frames idx of a row of pose_lds_cases (which share f, level and pos) as a batch"""
    idx = list(idx)
    B = len(idx)
    return dict(ns=row["ns"], n=row["n"][idx].copy(), f=np.tile(row["f"], (B, 1, 1)), level=np.tile(row["level"], (B, 1)),
                pos=np.tile(row["pos"], (B, 1, 1)), hp=row["hp"][idx].copy(), T0=row["T0"][idx].reshape(B, 12).copy(),
                what=[row["what"][i] for i in idx])


def take(batch, idx):
    idx = list(idx)
    return dict(ns=batch["ns"], what=[batch["what"][i] for i in idx],
                **{k: np.ascontiguousarray(batch[k][idx]) for k in ("n", "f", "level", "pos", "hp", "T0")})


def chunks(B, total=cases.B):
    """[0, total) in launches of B frames; the last one takes what is left"""
    return [range(lo, min(lo + B, total)) for lo in range(0, total, B)]


def run_in_chunks(run, row, B):
    """the sixteen frames of a row through launches of B frames each -> (T [16,12], Cov, stats, ran, hp) as one launch returns them"""
    parts = [run(from_row(row, c)) for c in chunks(B)]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(5))


def oracle_batch(orc, scene, batch, n_iter=cases.N_ITER):
    n = batch["n"]
    return [orc.pose_optimize(scene.cam, batch["T0"][b], batch["f"][b, :n[b]], batch["level"][b, :n[b]], batch["hp"][b, :n[b]],
                              batch["pos"][b, :n[b]], cases.THRESH, n_iter) for b in range(len(n))]


def mixed_batch(orc, scene, row):
    """-> (batch of nine frames at n_stride = 200, the oracle's answers).  row: pose_lds_cases.make_row(scene, 200)."""
    ns = 200
    assert row["ns"] == ns
    rng = fuzz_rng(4200)
    T_true = np.asarray(scene.T_f_w[scene.cur], np.float64).reshape(12)
    ordinary = from_row(row, range(cases.B - 4, cases.B))  # 193 live, all 200 live, twice 20 % dead at random
    frames = []

    def add(what, n, f, level, pos, hp, T0):
        frames.append(dict(what=what, n=n, f=f, level=level, pos=pos, hp=hp, T0=np.asarray(T0, np.float64).reshape(12)))

    f0, lv0, pos0, T0 = row["f"], row["level"], row["pos"], row["T0"].reshape(-1, 12)
    add("n_is_0", 0, f0, lv0, pos0, np.ones(ns, np.uint8), T0[1])                  # (flags beyond n: to come back untouched)
    add("no_flag_set", ns, f0, lv0, pos0, np.zeros(ns, np.uint8), T0[2])
    one = np.zeros(ns, np.uint8)
    one[77] = 1
    add("one_live_singular", ns, f0, lv0, pos0, one, T0[3])
    # observations at the exact projection of the scene's points under T_true, the start 1e-6 off: one step lands, the next is < 1e-10
    R, t = T_true[:9].reshape(3, 3), T_true[9:]
    pc = scene.pt_pos[:ns] @ R.T + t
    add("exact_projection", ns, pc / np.linalg.norm(pc, axis=1, keepdims=True), np.zeros(ns, np.int32), scene.pt_pos[:ns].copy(),
        np.ones(ns, np.uint8), se3.mul(se3.exp(rng.normal(size=6) * 1e-6), T_true))
    # gross outliers (35 % of the points 0.3 off, 0.5 px on the rest, the start 2e-2 off): the first draw on which the oracle
    # neither converges nor rolls back before the cap
    for k in range(200):
        r = fuzz_rng(4300 + k)
        f = synth._bearing(scene.cam, scene.px_true[:ns] + r.normal(size=(ns, 2)) * 0.5)
        pos = scene.pt_pos[:ns].copy()
        bad = r.uniform(size=ns) < 0.35
        pos[bad] += r.normal(size=(int(bad.sum()), 3)) * 0.3
        lv = r.integers(0, 3, size=ns).astype(np.int32)
        Ts = se3.mul(se3.exp(r.normal(size=6) * 2e-2), T_true)
        if orc.pose_optimize(scene.cam, Ts, f, lv, np.ones(ns, np.uint8), pos, cases.THRESH, cases.N_ITER)["n_iter_done"] == cases.N_ITER:
            add(f"all_ten_iterations_draw_{k}", ns, f, lv, pos, np.ones(ns, np.uint8), Ts)
            break
    else:
        raise AssertionError("no draw on which the oracle runs all ten iterations")
    for b in range(4):
        add("ordinary_" + ordinary["what"][b], ordinary["n"][b], ordinary["f"][b], ordinary["level"][b], ordinary["pos"][b],
            ordinary["hp"][b], ordinary["T0"][b])
    batch = dict(ns=ns, what=[fr["what"] for fr in frames], n=np.array([fr["n"] for fr in frames], np.int32),
                 f=np.stack([fr["f"] for fr in frames]).astype(np.float64), level=np.stack([fr["level"] for fr in frames]).astype(np.int32),
                 pos=np.stack([fr["pos"] for fr in frames]).astype(np.float64), hp=np.stack([fr["hp"] for fr in frames]).astype(np.uint8),
                 T0=np.stack([fr["T0"] for fr in frames]))
    return batch, oracle_batch(orc, scene, batch)


def check_mixed_classes(batch, want, ran_deferred):
    """the nine frames are what their names say: by the oracle (which ran, how many iterations updated the model) and by what
    the wave kernel's own launch leaves in `ran` (svo_hip_pose_optimize_deferred: 2 = handed over)"""
    it = [o["n_iter_done"] for o in want]
    assert [o["ran"] for o in want] == [0, 0, 1, 1, 1, 1, 1, 1, 1], batch["what"]
    assert int(batch["hp"][2, :batch["n"][2]].sum()) == 1  # two equations for six unknowns: the normal matrix has rank <= 2
    assert 1 <= it[3] <= 2, it      # stops early: converged (the second step is below 1e-10)
    assert it[4] == cases.N_ITER, it  # reaches the cap: ten updates, no roll-back
    assert all(1 <= k < cases.N_ITER for k in it[5:]), it
    assert tuple(int(r) for r in ran_deferred) == MIXED_RAN_DEFERRED, (ran_deferred, batch["what"])


def check_frames(batch, want, T, Cov, stats, ran, hp_out):
    """the requirements of pose_lds_cases.check (tracking_cases.check_pose) frame by frame, for a batch whose frames have their
    own observations"""
    check_pose(batch["n"], batch["hp"], batch["T0"], want, T, Cov, stats, ran, hp_out, beyond_n=True, tight_stats_live=0, what=batch["what"])


def width_frames(row):
    """the frames of the 256-slot row with WIDTH_COUNTS live observations, in that order"""
    assert row["ns"] == 256
    idx = [next(i for i, w in enumerate(row["what"]) if w.startswith(f"{c}_live_")) for c in WIDTH_COUNTS]
    assert [int(row["hp"][i, :row["n"][i]].sum()) for i in idx] == list(WIDTH_COUNTS)
    return idx


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_alone_equals_batch(run, batch, got):
    """every frame of the batch run alone (B = 1) returns the bytes it has in `got`, the batch's results: T, Cov, stats, ran and
    its row of has_point"""
    for b in range(len(batch["n"])):
        alone = run(take(batch, [b]))
        for name, x, y in zip(("T", "Cov", "stats", "ran", "has_point"), alone, got):
            assert same_bytes(x[0], y[b]), (b, batch["what"][b], name)
