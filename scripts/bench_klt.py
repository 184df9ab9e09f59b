#!/usr/bin/env python
"""Times the bootstrap's tracker (svo_hip_klt_track + svo_hip_klt_summarize, csrc/klt_track.hip) on rendered VGA frames
resident in HBM and writes profiles/klt_bench.json:

  (a) one pair x 352 points    a single camera's bootstrap frame: launch-bound, reported as such
  (b) 4096 pairs x 352 points  the replay shape

Call times are device events around one call after a warm-up; the kernel time of (b) comes from a `rocprofv3
--kernel-trace --stats` run of its own (this script started again with --traced-child); registers / scratch / occupancy
from the compiler's resource-usage remarks; mean iterations per point and level from the f64 checker
(tests/klt_checker.py) on a sample of the same problems.  Algorithmic bytes and operations are computed from the shapes
and those iteration counts; the kernel is placed against the larger of operations / peak rate and bytes / peak bandwidth.
The numpy checker is also timed on 352 points, labelled "f64 checker, not a baseline": the reference does this step
with OpenCV on the CPU, which is not part of this repository.  Needs an MI355X: there is no CPU path."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_F32_OPS = 157.3e12   # vector f32, an FMA counted as two (MI355X specification)
PEAK_HBM_BYTES = 8.0e12
W, LEVELS = 30, 5


def algorithmic_cost(iters_per_level, residual_evals=1.0):
    """(window bytes, f32 operations) one point needs, from the window size and the evaluations per level.
    Template (once per level): (W + 3)^2 reference pixels; Scharr x and y on the (W + 1)^2 grid (16 operations per
    position); per window pixel three bilinear samples (7 each), two scalings and the three tensor sums (6).
    Evaluation (per iteration, and once for the residual): (W + 1)^2 current pixels; per window pixel one bilinear
    sample (7), the difference (1) and two products summed (4).  A multiply and an add count as two operations, fused
    or not.  The windows of a pair's 352 points cover its two images about once and overlap from iteration to
    iteration, so the window bytes are what the caches serve; what HBM has to deliver is every pyramid the batch
    names, once, plus the points' own records (memory_bytes)."""
    evals = sum(iters_per_level) + residual_evals
    window_bytes = LEVELS * (W + 3) ** 2 + evals * (W + 1) ** 2
    ops = LEVELS * ((W + 1) ** 2 * 16 + W * W * (21 + 2 + 6)) + evals * W * W * 12
    return window_bytes, ops


def memory_bytes(n_pairs, n_pts, n_distinct_slots, pyramid_bytes):
    """px_ref 8 + px_cur in and out 16 + status in and out 2 + error 4 per point, two slot indices per pair"""
    return n_distinct_slots * pyramid_bytes + n_pairs * n_pts * 30 + n_pairs * 8


def compiler_resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        from rpg_svo_amd.build import FLAGS
        r = subprocess.run([hipcc, *FLAGS, "-c", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rpg_svo_amd", "csrc"),
                            os.path.join(ROOT, "rpg_svo_amd", "csrc", "klt_track.hip"), "-o", os.path.join(tmp, "klt.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    out = {}
    for blk in r.stderr.split("Function Name: ")[1:]:
        name = "klt_track_kernel" if "klt_track_kernel" in blk.split()[0] else "klt_summarize_kernel" if "klt_summarize_kernel" in blk.split()[0] else None
        if name and name not in out:
            g = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
            out[name] = {"vgprs": g("VGPRs"), "agprs": g("AGPRs"), "sgprs": g("TotalSGPRs"), "scratch_bytes_per_lane": g(r"ScratchSize \[bytes/lane\]"),
                         "occupancy_waves_per_simd": g(r"Occupancy \[waves/SIMD\]"), "lds_bytes_per_block": g(r"LDS Size \[bytes/block\]")}
    return out or "not measured"


class Problem:
    """n_pairs x n_pts problems on frames 1..8 of a rendered scene against its frame 0, the store copied `copies` times so
    that the pairs of a large batch do not all read the same nine pyramids out of the caches."""

    def __init__(self, dev, copies):
        import numpy as np
        import torch
        import klt_scenes
        from rpg_svo_amd import synth
        from rpg_svo_amd.pyramid import PyramidStore
        s = klt_scenes.make_scene(12345, 0.03, 9)
        self.scene, self.copies, self.dev = s, copies, dev
        self.px0 = synth.select_features(torch.from_numpy(s.images[:1]), 352, margin=28, cell=24)[0].numpy().astype(np.float32)
        self.store = PyramidStore(640, 480, LEVELS, 9 * copies, device=dev)
        imgs = torch.from_numpy(s.images).to(dev)
        for c in range(copies):
            self.store.load_images(imgs, first_slot=9 * c)
        torch.cuda.synchronize()

    def batch(self, n_pairs, n_pts):
        import numpy as np
        import torch
        p = np.arange(n_pairs)
        base = 9 * (p % self.copies)
        t = lambda a, dt: torch.as_tensor(np.array(a, order="C"), dtype=dt, device=self.dev)
        return (t(base, torch.int32), t(base + 1 + (p // self.copies) % 8, torch.int32),
                t(np.broadcast_to(self.px0[:n_pts], (n_pairs, n_pts, 2)), torch.float32))


def time_shape(prob, n_pairs, n_pts, steps, warmup):
    import torch
    from rpg_svo_amd.initialization import klt_track, klt_summarize, klt_params
    ref_slot, cur_slot, px_ref = prob.batch(n_pairs, n_pts)
    params = klt_params()
    px_cur, status = px_ref.clone(), torch.ones(n_pairs, n_pts, dtype=torch.uint8, device=prob.dev)
    error = torch.zeros(n_pairs, n_pts, dtype=torch.float32, device=prob.dev)
    t_track, t_both = [], []
    for i in range(warmup + steps):
        px_cur.copy_(px_ref)      # the call works in place: every step starts from "no motion"
        status.fill_(1)
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        klt_track(prob.store, ref_slot, cur_slot, px_ref, px_cur, status, error, params)
        e1.record()
        klt_summarize(prob.scene.cam, px_ref, px_cur, status)
        e2.record()
        torch.cuda.synchronize()
        if i >= warmup:
            t_track.append(e0.elapsed_time(e1))
            t_both.append(e0.elapsed_time(e2))
    t_track.sort()
    t_both.sort()
    med = t_track[len(t_track) // 2]
    return {"pairs": n_pairs, "points": n_pts, "steps": steps, "track_ms_median": med, "track_ms_min": t_track[0], "track_ms_max": t_track[-1],
            "track_and_summarize_ms_median": t_both[len(t_both) // 2], "points_per_s": n_pairs * n_pts / (med * 1e-3),
            "tracked_fraction": float(status.float().mean().item())}


def checker_sample(prob, n_sample_pts=8):
    """Iterations per point and level of the f64 checker on points of all eight pairs, and its time on 352 points."""
    import numpy as np
    import klt_checker
    pyr = lambda slot: [prob.store.level(slot, l) for l in range(LEVELS)]
    ref = pyr(0)
    its, evals = [], []
    for k in range(1, 9):
        sel = prob.px0[(k - 1)::44][:n_sample_pts]
        _, st, _, it = klt_checker.track(ref, pyr(k), sel, sel, np.ones(len(sel), np.uint8))
        its.append(it)
    its = np.concatenate(its)
    t0 = time.perf_counter()
    klt_checker.track(ref, pyr(4), prob.px0, prob.px0, np.ones(len(prob.px0), np.uint8))
    sec = time.perf_counter() - t0
    return its.mean(axis=0).tolist(), int(len(its)), sec


def traced_kernel_ms(args):
    """Kernel time of shape (b) from rocprofv3's kernel trace, in a run of its own."""
    out = tempfile.mkdtemp(prefix="klt_trace_", dir=os.path.join(ROOT, "build"))
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "trace", "--", sys.executable,
           os.path.abspath(__file__), "--traced-child", "--pairs", str(args.pairs), "--copies", str(args.copies)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
        return {"error": f"rocprofv3 exit {r.returncode}: {r.stderr[-400:]}"}
    res = {}
    for row in csv.DictReader(open(files[0])):
        name = row.get("Name", "")
        for k in ("klt_track_kernel", "klt_summarize_kernel"):
            if k in name:
                res[k] = {"calls": int(row["Calls"]), "average_ms": float(row["AverageNs"]) * 1e-6, "min_ms": float(row["MinNs"]) * 1e-6,
                          "max_ms": float(row["MaxNs"]) * 1e-6}
    return res or {"error": "no klt kernel in the trace"}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--copies", type=int, default=128, help="copies of the nine pyramids the pairs are spread over")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-compiler", action="store_true", help="skip the compile that reports registers, scratch and occupancy")
    ap.add_argument("--traced-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "klt_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_klt.py needs an MI355X: nothing here is measured without one")
    dev = torch.device("cuda:0")
    prob = Problem(dev, args.copies)
    if args.traced_child:
        time_shape(prob, args.pairs, 352, 3, 1)
        return
    res = {"device": torch.cuda.get_device_name(0), "window": W, "levels": LEVELS}
    res["single_pair"] = time_shape(prob, 1, 352, max(args.steps, 50), 5)
    res["single_pair"]["note"] = "launch-bound: 352 waves on 256 CUs, one launch"
    res["replay_batch"] = time_shape(prob, args.pairs, 352, args.steps, args.warmup)
    iters, n_sample, checker_sec = checker_sample(prob)
    res["checker_iterations_per_point_by_level"] = iters
    res["checker_iterations_per_point_and_level"] = sum(iters) / len(iters)
    res["checker_sample_points"] = n_sample
    res["f64_checker_not_a_baseline"] = {"points": 352, "seconds": checker_sec, "points_per_s": 352 / checker_sec}
    res["compiler"] = "not measured" if args.no_compiler else compiler_resources()
    res["rocprofv3"] = "not measured" if args.no_trace else traced_kernel_ms(args)
    window_bytes, ops = algorithmic_cost(iters)
    n = args.pairs * 352
    n_bytes = memory_bytes(args.pairs, 352, min(9 * args.copies, 9 * args.pairs), prob.store.bytes_per_pyramid()) / n
    kern = res["rocprofv3"].get("klt_track_kernel", {}).get("average_ms") if isinstance(res["rocprofv3"], dict) else None
    t_ms = kern if kern else res["replay_batch"]["track_ms_median"]
    t_ops, t_bytes = n * ops / PEAK_F32_OPS, n * n_bytes / PEAK_HBM_BYTES
    res["roofline"] = {"hbm_bytes_per_point": n_bytes, "window_bytes_per_point_from_caches": window_bytes,
                       "achieved_window_bytes_per_s": n * window_bytes / (t_ms * 1e-3), "f32_ops_per_point": ops, "time_basis": "rocprofv3 kernel time" if kern else "device events",
                       "time_ms": t_ms, "achieved_f32_ops_per_s": n * ops / (t_ms * 1e-3), "achieved_hbm_bytes_per_s": n * n_bytes / (t_ms * 1e-3),
                       "least_ms_by_operations": t_ops * 1e3, "least_ms_by_bytes": t_bytes * 1e3,
                       "bound": "f32 operations" if t_ops >= t_bytes else "HBM bytes", "share_of_bound": max(t_ops, t_bytes) * 1e3 / t_ms}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
