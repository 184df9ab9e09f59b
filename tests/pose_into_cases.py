"""TEST INFRASTRUCTURE, not a test.  The cases of tests/test_pose_into_emulated.py and tests/test_pose_into_gpu.py:
svo_hip_pose_optimize_into (include/svo_hip.h: the flags and the poses read where they are, the results written elsewhere) must
leave, byte for byte, what copying the inputs and calling svo_hip_pose_optimize on the copies leaves; the fix-up launch behind
both (one workgroup of csrc/pose_optimizer.hip's pose_opt_flagged_kernel looks at 64 words of `ran`) must finish exactly the
frames the wave kernel handed over; and the wave kernel's compaction (csrc/pose_optimizer_wave.hip) must not depend on which
trips of the row hold the live slots.  Frames and rows come from tests/pose_lds_cases.py and tests/pose_wg_map_cases.py.

A backend (the emulated library on host memory, the GPU library on device memory) gives: lib (the entries bound to
capi.PROTOTYPES), up(array) -> a buffer of its own holding the array's bytes, down(buffer, dtype, count, offset_bytes) -> numpy,
addr(buffer) -> int, sync().  Everything else is here, once.

call_into runs the new entry with its outputs in poisoned buffers between guard bands: whatever the entry does not write stays
0xA5 and differs from what the old entry leaves (flags are 0 or 1, no double of a pose is 0xA5A5A5A5A5A5A5A5)."""
import ctypes as C

import numpy as np

import pose_lds_cases as cases
import pose_wg_map_cases as wg
from helpers import fuzz_rng
from rpg_svo_amd import capi

ENTRIES = ("svo_hip_pose_optimize", "svo_hip_pose_optimize_deferred", "svo_hip_pose_optimize_ordered", "svo_hip_pose_optimize_into")
GUARD = 256                     # bytes of 0xA5 on either side of has_point_out and T_out
BATCH_SIZES = (1, 8, 200)
ROWS = (64, 200, 250, 256, 257)  # 257: beyond the wave kernel (POSE_WAVE_MAX_STRIDE = 256), the ordered kernel whatever the entry
NAMES = ("T", "Cov", "stats", "ran", "has_point")


def stretch(batch, B, cheap=(0, 1)):
    """B frames of the batch: all of them first; where B is larger all of them again at the end, and in between the frames `cheap`
    in turn (of mixed_batch: n = 0 and no flag set, which leave the kernel at once)"""
    nb = len(batch["n"])
    if B <= nb:
        return wg.take(batch, range(B))
    assert B >= 2 * nb
    return wg.take(batch, [*range(nb), *[cheap[i % len(cheap)] for i in range(B - 2 * nb)], *range(nb)])


def _inputs(be, batch):
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
    B, ns = len(batch["n"]), batch["ns"]
    host = dict(n=c(batch["n"], np.int32), f=c(batch["f"], np.float64).reshape(B, ns, 3), level=c(batch["level"], np.int32).reshape(B, ns),
                pos=c(batch["pos"], np.float64).reshape(B, ns, 3), hp=c(batch["hp"], np.uint8).reshape(B, ns),
                T0=c(batch["T0"], np.float64).reshape(B, 12))
    return B, ns, host, {k: be.up(v) for k, v in host.items()}


def _results(B):
    # what an exit that writes nothing leaves behind must be the same on both sides: the same start for Cov, stats and ran
    return np.zeros((B, 36)), np.zeros((B, 4)), np.full(B, -1, np.int32)


def call_in_place(be, cam, batch, n_iter=cases.N_ITER, entry="svo_hip_pose_optimize"):
    """copies of the flags and the poses, then the in-place entry on them -> (T, Cov, stats, ran, has_point)"""
    B, ns, host, d = _inputs(be, batch)
    T, hp = be.up(host["T0"]), be.up(host["hp"])
    Cov, stats, ran = (be.up(x) for x in _results(B))
    cs = capi.camera(cam)
    rc = getattr(be.lib, entry)(C.byref(cs), B, be.addr(d["n"]), ns, be.addr(d["f"]), be.addr(d["level"]), be.addr(d["pos"]), be.addr(hp),
                                cases.THRESH, n_iter, be.addr(T), be.addr(Cov), be.addr(stats), be.addr(ran), None)
    assert rc == 0, rc
    be.sync()
    return (be.down(T, np.float64, B * 12).reshape(B, 12), be.down(Cov, np.float64, B * 36).reshape(B, 36),
            be.down(stats, np.float64, B * 4).reshape(B, 4), be.down(ran, np.int32, B), be.down(hp, np.uint8, B * ns).reshape(B, ns))


def call_into(be, cam, batch, n_iter=cases.N_ITER, alias=False):
    """svo_hip_pose_optimize_into -> (T, Cov, stats, ran, has_point).  alias=False: the outputs are poisoned buffers between guard
    bands, and the guards and the inputs are checked here; alias=True: d_has_point_out == d_has_point_in and d_T_out == d_T_in,
    inside one guarded buffer each."""
    B, ns, host, d = _inputs(be, batch)
    poison = lambda nbytes: np.full(nbytes + 2 * GUARD, 0xA5, np.uint8)
    raw_hp, raw_T = poison(B * ns), poison(B * 96)
    if alias:
        raw_hp[GUARD:GUARD + B * ns] = host["hp"].ravel()
        raw_T[GUARD:GUARD + B * 96] = host["T0"].ravel().view(np.uint8)
    out_hp, out_T = be.up(raw_hp), be.up(raw_T)
    in_hp = be.addr(out_hp) + GUARD if alias else be.addr(d["hp"])
    in_T = be.addr(out_T) + GUARD if alias else be.addr(d["T0"])
    Cov, stats, ran = (be.up(x) for x in _results(B))
    cs = capi.camera(cam)
    rc = be.lib.svo_hip_pose_optimize_into(C.byref(cs), B, be.addr(d["n"]), ns, be.addr(d["f"]), be.addr(d["level"]), be.addr(d["pos"]),
                                           in_hp, in_T, cases.THRESH, n_iter, be.addr(out_hp) + GUARD, be.addr(out_T) + GUARD,
                                           be.addr(Cov), be.addr(stats), be.addr(ran), None)
    assert rc == 0, rc
    be.sync()
    got_hp, got_T = be.down(out_hp, np.uint8, len(raw_hp)), be.down(out_T, np.uint8, len(raw_T))
    for raw in (got_hp, got_T):
        assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all(), "a guard band was written"
    for k, v in host.items():  # the inputs: read only
        assert wg.same_bytes(be.down(d[k], v.dtype, v.size).reshape(v.shape), v), k
    return (got_T[GUARD:-GUARD].view(np.float64).reshape(B, 12).copy(), be.down(Cov, np.float64, B * 36).reshape(B, 36),
            be.down(stats, np.float64, B * 4).reshape(B, 4), be.down(ran, np.int32, B), got_hp[GUARD:-GUARD].reshape(B, ns).copy())


def assert_same(got, want, what):
    for name, x, y in zip(NAMES, got, want):
        if not wg.same_bytes(x, y):
            x, y = np.asarray(x).reshape(len(x), -1), np.asarray(y).reshape(len(y), -1)
            bad = [b for b in range(len(x)) if x[b].tobytes() != y[b].tobytes()]
            raise AssertionError((what, name, "frames", bad[:10]))


def check_into(be, cam, batch, n_iter=cases.N_ITER, what=""):
    """the new entry against copy + the old one, byte for byte: into fresh buffers, and in place -> the old entry's results"""
    want = call_in_place(be, cam, batch, n_iter)
    assert_same(call_into(be, cam, batch, n_iter), want, (what, "into"))
    assert_same(call_into(be, cam, batch, n_iter, alias=True), want, (what, "in == out"))
    return want


# ---- the `ran` scan of the fix-up launch ---------------------------------------------------------------------------------------
SCAN_NS = 64
# (B, the frames handed over)
SCAN_CASES = {"first_of_a_chunk": (128, (64,)), "first_of_the_batch": (128, (0,)), "last_of_a_chunk": (128, (63,)),
              "around_a_boundary": (192, (63, 64)), "two_in_one_chunk": (128, (70, 71)), "partial_chunk_of_1": (65, (64,)),
              "partial_chunk_of_63": (127, (126,)), "partial_chunk_after_two": (129, (128,)), "chunk_of_1_and_first": (129, (0, 127, 128)),
              "none": (129, ())}


def scan_batch(scene, B, flagged):
    """B frames of SCAN_NS slots.  At the places `flagged` a frame with one live observation, its own slot and start each -- two
    equations for six unknowns, which the wave kernel hands over (ran = 2); on either side of each of them, at both ends of the
    batch and on both sides of every chunk boundary an ordinary frame (the 20-percent-dead frames of the row, which the wave kernel
    takes: the neighbours whose results must not move); everywhere else a frame without a flag (ran = 0, the pose and the flags as
    they came in), which costs the emulation nothing."""
    row = cases.make_row(scene, SCAN_NS)
    ordinary = [i for i, w in enumerate(row["what"]) if w.startswith("20_percent_dead")]
    batch = wg.from_row(row, [ordinary[i % len(ordinary)] for i in range(B)])
    keep = {0, B - 1} | {b + d for b in flagged for d in (-1, 1)} | {c + d for c in range(64, B, 64) for d in (-1, 0)}
    for b in range(B):
        if b not in keep:
            batch["hp"][b] = 0
            batch["what"][b] = "no_flag_set"
    rng = fuzz_rng(5200 + B)
    for b in flagged:
        batch["hp"][b] = 0
        batch["hp"][b, int(rng.integers(0, SCAN_NS))] = 1
        batch["T0"][b] = row["T0"].reshape(-1, 12)[int(rng.integers(0, cases.B))]
        batch["what"][b] = "one_live_singular"
    return batch


def check_scan(be, cam, batch, flagged):
    """svo_hip_pose_optimize and _into: the flagged frames as svo_hip_pose_optimize_ordered leaves them, every other frame as the
    wave kernel alone (the deferred entry) leaves it"""
    B = len(batch["n"])
    deferred = call_in_place(be, cam, batch, entry="svo_hip_pose_optimize_deferred")
    assert sorted(np.flatnonzero(deferred[3] == 2).tolist()) == sorted(flagged), deferred[3].tolist()
    want = [x.copy() for x in deferred]
    if flagged:
        sub = call_in_place(be, cam, wg.take(batch, flagged), entry="svo_hip_pose_optimize_ordered")
        for x, y in zip(want, sub):
            x[list(flagged)] = y
        assert (sub[3] == 1).all()
    assert_same(call_in_place(be, cam, batch), want, "svo_hip_pose_optimize")
    assert_same(call_into(be, cam, batch), want, "svo_hip_pose_optimize_into")


# ---- where the live slots sit in the row (the wave kernel's compaction) ---------------------------------------------------------
def layout_batch(scene):
    """frames of 256 slots: the live slots only in the last trip (slots 192 ..); n = 1, 64, 65 and 193 with EVERY flag of the row
    set (those at and beyond n are not the frame's); alternating flags, even and odd; only the last slot"""
    row = cases.make_row(scene, 256)
    ns, T0 = 256, row["T0"].reshape(-1, 12)
    frames = []

    def add(what, n, hp):
        frames.append((what, n, np.asarray(hp, np.uint8), T0[len(frames) % len(T0)]))

    last = np.zeros(ns, np.uint8)
    last[192:] = 1
    add("last_trip_only", ns, last)
    last_short = np.zeros(ns, np.uint8)
    last_short[192:] = 1
    add("last_trip_only_n_230", 230, last_short)
    for n in (1, 64, 65, 193):
        add(f"all_set_n_{n}", n, np.ones(ns, np.uint8))
    even = (np.arange(ns) % 2 == 0).astype(np.uint8)
    add("alternating_even", ns, even)
    add("alternating_odd", ns, 1 - even)
    add("alternating_odd_n_129", 129, 1 - even)
    only = np.zeros(ns, np.uint8)
    only[255] = 1
    add("last_slot_only", ns, only)
    B = len(frames)
    return dict(ns=ns, what=[fr[0] for fr in frames], n=np.array([fr[1] for fr in frames], np.int32), f=np.tile(row["f"], (B, 1, 1)),
                level=np.tile(row["level"], (B, 1)), pos=np.tile(row["pos"], (B, 1, 1)), hp=np.stack([fr[2] for fr in frames]),
                T0=np.stack([fr[3] for fr in frames]))
