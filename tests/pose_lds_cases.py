"""TEST INFRASTRUCTURE, not a test.  The table of tests/test_pose_lds_emulated.py and tests/test_pose_lds_gpu.py: rows of
n_stride observations for the wave kernel of the pose optimizer (csrc/pose_optimizer_wave.hip), which compacts a frame's live
observations into LDS and walks them in trips of 64.  Sixteen frames per row length:

  * live counts on every trip boundary the row can hold: 0, 1, 5, 20, 63, 64, 65, 127, 128, 129, 191, 192, 193, n_stride;
  * the live slots of a frame laid out by one of five patterns (PATTERN) -- a prefix of the row (the count n_stride: all
    live); slots 0..63 dead and the rest of the frame's n = 64 + count slots live (every observation moves, the index map
    decides where pruning lands); only slots >= 192 live, n = 192 + count; at random; n below n_stride with every flag beyond n
    set (those must be ignored and come back untouched);
  * the places left of the sixteen: ~20 % of the row dead at random;
  * every 15th point grossly wrong, as tests/test_tracking_gpu.py::test_pose_optimize has them, so that pruning fires.

check() compares one row's results with the oracle under the requirements of that test (tracking_cases.check_pose)."""
import numpy as np

from helpers import FUZZ, camera_models, fuzz_rng
from rpg_svo_amd import se3, synth
from tracking_cases import check_pose, check_pose_median

ROWS = (7, 64, 65, 200, 250, 256)
COUNTS = (0, 1, 5, 20, 63, 64, 65, 127, 128, 129, 191, 192, 193)
B = 16
N_ITER = 10
THRESH = 2.0
# which pattern lays out the frame of each live count: the first one the row can hold
PATTERN = {0: ("prefix",), 1: ("head_dead", "random"), 5: ("tail", "short_n"), 20: ("tail", "random"), 63: ("tail", "short_n"),
           64: ("tail", "head_dead", "prefix"), 65: ("head_dead", "prefix"), 127: ("random",), 128: ("head_dead", "prefix"),
           129: ("short_n",), 191: ("head_dead", "random"), 192: ("head_dead", "short_n"), 193: ("short_n",)}


def make_scene():
    return synth.make_track_scene(n_kf=4, n_feat=100, cam=camera_models()["pinhole"], seed=777 + FUZZ)


def _flags(kind, ns, c, rng):
    """-> (n, flags[ns]) with exactly c live observations among the first n slots, or None where the row cannot hold it"""
    hp = np.zeros(ns, np.uint8)
    n = ns
    if kind == "prefix":
        hp[:c] = 1
    elif kind == "head_dead":
        if 64 + c > ns:
            return None
        n = 64 + c  # (a frame of n observations: its slots 0..63 dead and the rest live)
        hp[64:n] = 1
    elif kind == "tail":
        if 192 + c > ns:
            return None
        n = 192 + c
        hp[192:n] = 1
    elif kind == "random":
        hp[rng.choice(ns, size=c, replace=False)] = 1
    elif kind == "short_n":
        n = max(c, ns - max(1, ns // 5))
        if n >= ns:
            return None
        hp[rng.choice(n, size=c, replace=False)] = 1
        hp[n:] = 1
    return n, hp


def make_row(scene, ns):
    """-> dict of the row's arrays: n [B], f [ns,3], level [ns], pos [ns,3], hp [B,ns], T0 [B,3,4], what [B] (a label per frame)"""
    rng = fuzz_rng(100 + ns)
    f = synth._bearing(scene.cam, scene.px_true[:ns] + rng.normal(size=(ns, 2)) * 0.3)
    level = rng.integers(0, 3, size=ns).astype(np.int32)
    pos = scene.pt_pos[:ns].copy()
    pos[::15] += rng.normal(size=pos[::15].shape) * 0.2
    frames = []
    for c in [c for c in COUNTS if c < ns] + [ns]:
        for kind in (("prefix",) if c == ns else PATTERN[c]):  # the first pattern that can hold c live observations in this row
            got = _flags(kind, ns, c, rng)
            if got is not None:
                frames.append((f"{c}_live_{kind}",) + got)
                break
    i = 0
    while len(frames) < B:
        frames.append((f"20_percent_dead_{i}", ns, (rng.uniform(size=ns) > 0.2).astype(np.uint8)))
        i += 1
    assert len(frames) == B
    T0 = np.stack([se3.mul(se3.exp(rng.normal(size=6) * 5e-3), scene.T_f_w[scene.cur]) for _ in range(B)])
    return dict(ns=ns, n=np.array([fr[1] for fr in frames], np.int32), f=f, level=level, pos=pos,
                hp=np.stack([fr[2] for fr in frames]), T0=T0, what=[fr[0] for fr in frames])


def oracle_row(orc, scene, row, n_iter=N_ITER):
    """the oracle's answer for every frame of the row (computed once per row and shared)"""
    n = row["n"]
    return [orc.pose_optimize(scene.cam, row["T0"][b], row["f"][:n[b]], row["level"][:n[b]], row["hp"][b, :n[b]], row["pos"][:n[b]],
                              THRESH, n_iter) for b in range(B)]


def moved_and_pruned(row, want):
    """frames in which the oracle prunes an observation that compaction moves (its position among the live ones differs from
    its slot): the kernel clears the right flag there only through the slot index it stored"""
    out = []
    for b in range(B):
        n = row["n"][b]
        if not want[b]["ran"]:
            continue
        before = row["hp"][b, :n].astype(bool)
        pruned = before & ~np.asarray(want[b]["has_point"]).astype(bool)
        at = np.cumsum(before) - 1
        if (pruned & (at != np.arange(n))).any():
            out.append(b)
    return out


def check(row, want, T, Cov, stats, ran, hp_out):
    """tracking_cases.check_pose (the requirements of tests/test_tracking_gpu.py::test_pose_optimize) on every frame that ran,
    none skipped on the committed scene, with the tight bound on scale and errors wherever the pose agrees to 1e-11; flags
    beyond n untouched; the median where a row has frames of 20 or more live observations"""
    devs = check_pose(row["n"], row["hp"], row["T0"], want, T, Cov, stats, ran, hp_out, beyond_n=True, tight_stats_live=0,
                      what=[(row["ns"], w) for w in row["what"]])
    if devs:
        check_pose_median(devs)
    return devs


# ---- the stand-alone sanitizer program (tests/host/pose_lds_asan_main.cpp): input file, output file ---------------------------
def write_rows(path, scene, rows):
    from rpg_svo_amd import capi
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt).tobytes()
    with open(path, "wb") as fh:
        for row in rows:
            ns = row["ns"]
            fh.write(c([ns, B, N_ITER], np.int32) + c([THRESH], np.float64) + bytes(capi.camera(scene.cam)))
            fh.write(c(row["n"], np.int32) + c(np.tile(row["f"], (B, 1, 1)), np.float64) + c(np.tile(row["level"], (B, 1)), np.int32)
                     + c(np.tile(row["pos"], (B, 1, 1)), np.float64) + c(row["hp"], np.uint8) + c(row["T0"], np.float64))


def read_results(path, rows):
    """-> per row a list of two (T, Cov, stats, ran, has_point): svo_hip_pose_optimize, and its deferred entry with n_iter = 0"""
    buf, at, out = open(path, "rb").read(), 0, []

    def take(dt, *shape):
        nonlocal at
        a = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape)), offset=at).reshape(shape)
        at += a.nbytes
        return a.copy()

    for row in rows:
        out.append([(take(np.float64, B, 12), take(np.float64, B, 36), take(np.float64, B, 4), take(np.int32, B), take(np.uint8, B, row["ns"]))
                    for _ in range(2)])
    assert at == len(buf)
    return out
