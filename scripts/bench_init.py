#!/usr/bin/env python
"""Times the bootstrap's homography step (svo_hip_homography_init, csrc/homography_init.hip) on synthetic two-view scenes
resident in HBM (tests/homography_cases.py: a plane with 3 % relief, 0.3 px noise, 30 % outliers, 352 tracked points) and
writes profiles/homography_bench.json:

  (a) one pair x 352 points    a single camera's bootstrap frame: one workgroup, launch- and latency-bound
  (b) 4096 pairs x 352 points  the replay shape, beside klt_track's 33.8 ms for the same batch (profiles/klt_bench.json)

Call times are device events around one call after a warm-up, median of 10; the kernel time of (b) comes from a
`rocprofv3 --kernel-trace --stats` run of its own (this script started again with --traced-child); registers / scratch /
occupancy from the compiler's resource-usage remarks.  The algorithmic f64 operation count is derived from the shapes
(operations() below) and the kernel is placed against operations / peak vector f64 rate.  Needs an MI355X: there is no
CPU path, and nothing is measured without one (the JSON then says "not measured").

--step first_map times what follows the homography step instead (svo_hip_first_map and svo_hip_initialize_seeds,
csrc/first_map.hip; the detector between them is K7's and is not timed here) on 1 x 416 and 4096 x 416 corners (the 26 x 16
grid of a 752 x 480 image, about 260 map points and 170 new corners per sequence) and writes profiles/first_map_bench.json:
the same device events, the two kernels' own times from the same kind of rocprofv3 run, and the bytes the step moves, from
the shapes, against the HBM rate.

--step frame_close times the end of a tracked frame (svo_hip_frame_close, csrc/frame_close.hip) on 1 and 4096 sequences x 121
rows x 10 keyframes (max_fts + 1 features, a full keyframe list) and writes profiles/frame_close_bench.json in the same
form: device events, the kernel's own time from a rocprofv3 run of its own, the compiler's figures and the bytes per sequence.

--step keyframe_insert times a keyframe entering the resident map (svo_hip_keyframe_insert, csrc/keyframe_insert.hip) on 4096
sequences of 10 keyframes x 121 features, about 1400 points and candidates, a removal and a handful of promotions each (16
distinct maps of tests/keyframe_insert_cases.py, repeated; the state is restored before every timed call) and writes
profiles/keyframe_insert_bench.json: device events, the kernel's own time from a rocprofv3 run, the compiler's figures and the
bytes moved, counted from the shapes, against the HBM rate."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_F64_OPS = 78.6e12    # vector f64, an FMA counted as two (MI355X specification)
KLT_TRACK_MS = 33.8       # svo_hip_klt_track, 4096 pairs x 352 points (profiles/klt_bench.json)
POINTS, DISTINCT = 352, 64
KERNEL = "homography_init_kernel"


def operations(m, n_hypotheses, refine_iters, inlier_share=0.7):
    """f64 operations one pair needs, a multiply, an add, a compare and a division each counted as one.
    Hypothesis: two projective bases (3 cross products 27, |p|^2 sum 20, determinant 5, lambda 15: 67 each), the three
    column factors 6, B adj(A) 54, nine divisions: 203.  Score per point: H x 12, reciprocal 1, projection and
    differences 4, squared norm 3, compare 1: 21.  Refinement per evaluation and inlier: H x 12, five divisions, residual
    2, the 30 products and sums 74: 93; an 8 x 8 LDL' with its substitutions about 400.  The inlier pass, the candidate
    scores (8 candidates x 7), triangulation (about 90) and the map points (about 40) are per point, once."""
    hyp = n_hypotheses * (203 + 21 * m)
    refine = (refine_iters + 1) * (93 * inlier_share * m) + refine_iters * 400
    rest = m * (21 + 56 + 90 + 40)
    return hyp + refine + rest


def compiler_resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        from rpg_svo_amd.build import FLAGS
        r = subprocess.run([hipcc, *FLAGS, "-c", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rpg_svo_amd", "csrc"),
                            os.path.join(ROOT, "rpg_svo_amd", "csrc", "homography_init.hip"), "-o", os.path.join(tmp, "hi.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    for blk in r.stderr.split("Function Name: ")[1:]:
        if KERNEL in blk.split()[0]:
            g = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
            return {"vgprs": g("VGPRs"), "agprs": g("AGPRs"), "sgprs": g("TotalSGPRs"), "scratch_bytes_per_lane": g(r"ScratchSize \[bytes/lane\]"),
                    "occupancy_waves_per_simd": g(r"Occupancy \[waves/SIMD\]"), "lds_bytes_per_block": g(r"LDS Size \[bytes/block\]")}
    return "not measured"


def make_inputs(dev, n_pairs):
    """n_pairs pairs of 352 tracked points: DISTINCT scenes, repeated"""
    import numpy as np
    import torch
    import homography_cases as cases
    pairs = [cases.make_pair(5000 + k, POINTS, n_lost=0) for k in range(min(DISTINCT, n_pairs))]
    b = cases._batch("bench", pairs)
    reps = -(-n_pairs // len(pairs))
    inp = {k: torch.from_numpy(np.tile(v, (reps,) + (1,) * (v.ndim - 1))[:n_pairs].copy()).to(dev) for k, v in cases.inputs(b).items()}
    return b.cam, inp


def time_shape(dev, n_pairs, steps, warmup):
    import torch
    from rpg_svo_amd import initialization as init
    cam, inp = make_inputs(dev, n_pairs)
    out = init.homography_outputs(n_pairs, POINTS, dev)
    params = init.homography_params()
    times = []
    for i in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        init.homography_init(cam, inp["f_ref"], inp["f_cur"], inp["status"], inp["px_ref"], inp["px_cur"], inp["T_ref_w"], params, out)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    times.sort()
    med = times[len(times) // 2]
    ops = operations(POINTS, params.n_hypotheses, params.refine_iters)
    return {"pairs": n_pairs, "points": POINTS, "n_hypotheses": int(params.n_hypotheses), "refine_iters": int(params.refine_iters), "steps": steps,
            "call_ms_median": med, "call_ms_min": times[0], "call_ms_max": times[-1], "pairs_per_s": n_pairs / (med * 1e-3),
            "success_fraction": float((out["result"] == 2).float().mean().item()),
            "ambiguous_fraction": float(out["ambiguous"].float().mean().item()),
            "mean_inliers": float(out["n_inliers"].float().mean().item()), "f64_ops_per_pair": ops}


def traced_kernel_ms(args):
    """Kernel time of shape (b) from rocprofv3's kernel trace, in a run of its own."""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    out = tempfile.mkdtemp(prefix="init_trace_", dir=os.path.join(ROOT, "build"))
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "trace", "--", sys.executable,
           os.path.abspath(__file__), "--traced-child", "--pairs", str(args.pairs)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
        return {"error": f"rocprofv3 exit {r.returncode}: {r.stderr[-400:]}"}
    for row in csv.DictReader(open(files[0])):
        if KERNEL in row.get("Name", ""):
            return {"calls": int(row["Calls"]), "average_ms": float(row["AverageNs"]) * 1e-6, "min_ms": float(row["MinNs"]) * 1e-6,
                    "max_ms": float(row["MaxNs"]) * 1e-6}
    return {"error": "the kernel is not in the trace"}


# ---- the first-map step (K10) ---------------------------------------------------------------------------------------------
PEAK_HBM_BYTES = 8.0e12   # bytes / s (MI355X specification)
CORNERS, GRID = 416, (30, 26, 16)
FIRST_MAP_KERNELS = ("first_map_kernel", "seed_init_kernel")


def first_map_bytes(n_pts, cells, share=0.625):
    """bytes one sequence moves through both kernels: every output element is written once, an input of a corner that is
    no map point is read only as far as its flag (share = the fraction of corners that become map points)"""
    read = 4 + n_pts + share * n_pts * (24 + 2 * 8 + 2 * 24) + 2 * 96 + 2 * share * n_pts * 2 * 8     # (the pixels twice more: key points)
    written = 4 + n_pts * (4 + 24 + 2 * 16 + 2 * 24 + 24) + 40 + 16 + cells
    seeds = cells * (8 + 4 + 4) + 20 + 4 + cells * (4 + 4 + 1 + 16 + 24 + 16 + 5 * 4 + 4)
    return read + written + seeds


def compiler_resources_first_map():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        from rpg_svo_amd.build import FLAGS
        r = subprocess.run([hipcc, *FLAGS, "-c", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rpg_svo_amd", "csrc"),
                            os.path.join(ROOT, "rpg_svo_amd", "csrc", "first_map.hip"), "-o", os.path.join(tmp, "fm.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    out = {}
    for blk in r.stderr.split("Function Name: ")[1:]:
        for kern in FIRST_MAP_KERNELS:
            if kern in blk.split()[0]:
                g = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
                out[kern] = {"vgprs": g("VGPRs"), "agprs": g("AGPRs"), "sgprs": g("TotalSGPRs"), "scratch_bytes_per_lane": g(r"ScratchSize \[bytes/lane\]"),
                             "occupancy_waves_per_simd": g(r"Occupancy \[waves/SIMD\]"), "lds_bytes_per_block": g(r"LDS Size \[bytes/block\]")}
    return out or "not measured"


def time_first_map(dev, n_seq, steps, warmup):
    import numpy as np
    import torch
    import first_map_cases as cases
    from rpg_svo_amd import initialization as init
    from rpg_svo_amd.tracking import DepthFilter
    cam = cases.camera(752, 480)
    distinct = min(DISTINCT, n_seq)
    b = cases._batch("bench", [cases.make_seq(cam, 7000 + k, CORNERS, 260) for k in range(distinct)], GRID[0])
    assert b.grid == GRID
    reps = -(-n_seq // distinct)
    tile = lambda v: torch.from_numpy(np.tile(v, (reps,) + (1,) * (v.ndim - 1))[:n_seq].copy()).to(dev)
    inp = [tile(v) for v in cases.inputs(b).values()]
    c = cases.make_corners(7100, distinct, CORNERS, 0.4, cam)
    corners = [tile(v) for v in (c.xy, c.level, c.score)]
    frame_index = torch.arange(n_seq, dtype=torch.int32, device=dev)
    fm, seeds = None, None
    times = {"first_map": [], "initialize_seeds": [], "both": []}
    for i in range(warmup + steps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        fm = init.first_map(cam, *inp, *GRID, fm)
        e[1].record()
        seeds = DepthFilter.initialize_seeds(cam, *corners, c.threshold, frame_index, fm.depth_mean, fm.depth_min, 1, out=seeds)
        e[2].record()
        torch.cuda.synchronize()
        if i >= warmup:
            times["first_map"].append(e[0].elapsed_time(e[1]))
            times["initialize_seeds"].append(e[1].elapsed_time(e[2]))
            times["both"].append(e[0].elapsed_time(e[2]))
    res = {"sequences": n_seq, "corners": CORNERS, "cells": CORNERS, "steps": steps, "mean_points": float(fm.n_points.float().mean().item()),
           "mean_seeds": float(seeds[2].float().mean().item()), "bytes_per_sequence": first_map_bytes(CORNERS, CORNERS)}
    for k, v in times.items():
        v.sort()
        res[k] = {"call_ms_median": v[len(v) // 2], "call_ms_min": v[0], "call_ms_max": v[-1]}
    res["sequences_per_s"] = n_seq / (res["both"]["call_ms_median"] * 1e-3)
    return res


def traced_first_map_ms(args):
    """Kernel times of the replay shape from rocprofv3's kernel trace, in a run of its own."""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    out = tempfile.mkdtemp(prefix="first_map_trace_", dir=os.path.join(ROOT, "build"))
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "trace", "--", sys.executable,
           os.path.abspath(__file__), "--step", "first_map", "--traced-child", "--pairs", str(args.pairs)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
        return {"error": f"rocprofv3 exit {r.returncode}: {r.stderr[-400:]}"}
    res = {}
    for row in csv.DictReader(open(files[0])):
        for kern in FIRST_MAP_KERNELS:
            if kern in row.get("Name", ""):
                res[kern] = {"calls": int(row["Calls"]), "average_ms": float(row["AverageNs"]) * 1e-6, "min_ms": float(row["MinNs"]) * 1e-6,
                             "max_ms": float(row["MaxNs"]) * 1e-6}
    return res or {"error": "the kernels are not in the trace"}


def main_first_map(args):
    import torch
    out = args.out or os.path.join(ROOT, "profiles", "first_map_bench.json")
    if not torch.cuda.is_available():
        res = {"device": "not measured", "single_sequence": "not measured", "replay_batch": "not measured", "rocprofv3": "not measured",
               "compiler": "not measured" if args.no_compiler else compiler_resources_first_map(),
               "bytes_per_sequence": first_map_bytes(CORNERS, CORNERS), "note": "no MI355X was available: nothing here is measured without one"}
    else:
        dev = torch.device("cuda:0")
        if args.traced_child:
            time_first_map(dev, args.pairs, 3, 1)
            return
        res = {"device": torch.cuda.get_device_name(0), "library": os.environ.get("SVO_HIP_LIB", "in-tree")}
        res["single_sequence"] = time_first_map(dev, 1, max(args.steps, 10), 5)
        res["single_sequence"]["note"] = "one workgroup per kernel: launch-bound"
        res["replay_batch"] = time_first_map(dev, args.pairs, args.steps, args.warmup)
        res["compiler"] = "not measured" if args.no_compiler else compiler_resources_first_map()
        res["rocprofv3"] = "not measured" if args.no_trace else traced_first_map_ms(args)
        kern = sum(v["average_ms"] for v in res["rocprofv3"].values()) if isinstance(res["rocprofv3"], dict) and "error" not in res["rocprofv3"] else None
        t_ms = kern if kern else res["replay_batch"]["both"]["call_ms_median"]
        nbytes = res["replay_batch"]["bytes_per_sequence"] * args.pairs
        res["hbm_bound"] = {"time_basis": "rocprofv3 kernel times, summed" if kern else "device events", "time_ms": t_ms, "bytes": nbytes,
                            "peak_bytes_per_s": PEAK_HBM_BYTES, "least_ms_by_bytes": nbytes / PEAK_HBM_BYTES * 1e3,
                            "achieved_bytes_per_s": nbytes / (t_ms * 1e-3), "share_of_bound": nbytes / PEAK_HBM_BYTES * 1e3 / t_ms,
                            "klt_track_ms_same_batch": KLT_TRACK_MS, "share_of_klt_track": t_ms / KLT_TRACK_MS}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


# ---- the end of a tracked frame (K11) -----------------------------------------------------------------------------------
ROWS, KEYFRAMES = 121, 10
FRAME_CLOSE_KERNEL = "frame_close_kernel"


def frame_close_bytes(rows, kfs, cells, share=0.7):
    """bytes one sequence moves: every output element is written once; a row's pixel is read for the occupancy and, where it
    has a point (share of the rows), twice more for the key points; position and bearing only where the row has a point"""
    read = 4 * 4 + 2 * 96 + rows * (1 + 16) + share * rows * (2 * 16 + 24 + 24) + kfs * (96 + 4)
    written = 6 * 4 + 96 + 2 * 8 + rows * (1 + 24) + 5 * 4 + cells
    return read + written


def compiler_resources_frame_close():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        from rpg_svo_amd.build import FLAGS
        r = subprocess.run([hipcc, *FLAGS, "-c", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rpg_svo_amd", "csrc"),
                            os.path.join(ROOT, "rpg_svo_amd", "csrc", "frame_close.hip"), "-o", os.path.join(tmp, "fc.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    for blk in r.stderr.split("Function Name: ")[1:]:
        if FRAME_CLOSE_KERNEL in blk.split()[0]:
            g = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
            return {"vgprs": g("VGPRs"), "agprs": g("AGPRs"), "sgprs": g("TotalSGPRs"), "scratch_bytes_per_lane": g(r"ScratchSize \[bytes/lane\]"),
                    "occupancy_waves_per_simd": g(r"Occupancy \[waves/SIMD\]"), "lds_bytes_per_block": g(r"LDS Size \[bytes/block\]")}
    return "not measured"


def time_frame_close(dev, n_seq, steps, warmup):
    import numpy as np
    import torch
    import first_map_cases
    import frame_close_cases as cases
    from rpg_svo_amd import tracking as tr
    cam = first_map_cases.camera(752, 480)
    distinct = min(DISTINCT, n_seq)
    b = cases._batch("bench", [cases.make_seq(cam, 8000 + k, ROWS, ROWS, n_kf=KEYFRAMES, kf_stride=KEYFRAMES, num_obs=85, num_obs_last=100)
                               for k in range(distinct)], GRID[0])
    assert b.grid == GRID
    reps = -(-n_seq // distinct)
    inp = [torch.from_numpy(np.tile(v, (reps,) + (1,) * (v.ndim - 1))[:n_seq].copy()).to(dev) for v in cases.inputs(b).values()]
    out, times = None, []
    for i in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = tr.close_frame(cam, *inp, *GRID, out=out)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    times.sort()
    med = times[len(times) // 2]
    return {"sequences": n_seq, "rows": ROWS, "keyframes": KEYFRAMES, "cells": GRID[1] * GRID[2], "steps": steps, "call_ms_median": med,
            "call_ms_min": times[0], "call_ms_max": times[-1], "sequences_per_s": n_seq / (med * 1e-3),
            "mean_points": float(out.nobs_out.float().mean().item()), "keyframe_fraction": float((out.result == 1).float().mean().item()),
            "bytes_per_sequence": frame_close_bytes(ROWS, KEYFRAMES, GRID[1] * GRID[2])}


def traced_frame_close_ms(args):
    """Kernel time of the replay shape from rocprofv3's kernel trace, in a run of its own."""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    out = tempfile.mkdtemp(prefix="frame_close_trace_", dir=os.path.join(ROOT, "build"))
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "trace", "--", sys.executable,
           os.path.abspath(__file__), "--step", "frame_close", "--traced-child", "--pairs", str(args.pairs)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
        return {"error": f"rocprofv3 exit {r.returncode}: {r.stderr[-400:]}"}
    for row in csv.DictReader(open(files[0])):
        if FRAME_CLOSE_KERNEL in row.get("Name", ""):
            return {"calls": int(row["Calls"]), "average_ms": float(row["AverageNs"]) * 1e-6, "min_ms": float(row["MinNs"]) * 1e-6,
                    "max_ms": float(row["MaxNs"]) * 1e-6}
    return {"error": "the kernel is not in the trace"}


def main_frame_close(args):
    import torch
    out = args.out or os.path.join(ROOT, "profiles", "frame_close_bench.json")
    nbytes = frame_close_bytes(ROWS, KEYFRAMES, GRID[1] * GRID[2])
    if not torch.cuda.is_available():
        res = {"device": "not measured", "single_sequence": "not measured", "replay_batch": "not measured", "rocprofv3": "not measured",
               "compiler": "not measured" if args.no_compiler else compiler_resources_frame_close(), "bytes_per_sequence": nbytes,
               "note": "no MI355X was available: nothing here is measured without one"}
    else:
        dev = torch.device("cuda:0")
        if args.traced_child:
            time_frame_close(dev, args.pairs, 3, 1)
            return
        res = {"device": torch.cuda.get_device_name(0), "library": os.environ.get("SVO_HIP_LIB", "in-tree")}
        res["single_sequence"] = time_frame_close(dev, 1, max(args.steps, 10), 5)
        res["single_sequence"]["note"] = "one workgroup: launch-bound"
        res["replay_batch"] = time_frame_close(dev, args.pairs, args.steps, args.warmup)
        res["compiler"] = "not measured" if args.no_compiler else compiler_resources_frame_close()
        res["rocprofv3"] = "not measured" if args.no_trace else traced_frame_close_ms(args)
        kern = res["rocprofv3"].get("average_ms") if isinstance(res["rocprofv3"], dict) else None
        t_ms = kern if kern else res["replay_batch"]["call_ms_median"]
        res["hbm_bound"] = {"time_basis": "rocprofv3 kernel time" if kern else "device events", "time_ms": t_ms, "bytes": nbytes * args.pairs,
                            "peak_bytes_per_s": PEAK_HBM_BYTES, "least_ms_by_bytes": nbytes * args.pairs / PEAK_HBM_BYTES * 1e3,
                            "achieved_bytes_per_s": nbytes * args.pairs / (t_ms * 1e-3), "share_of_bound": nbytes * args.pairs / PEAK_HBM_BYTES * 1e3 / t_ms}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


# ---- a keyframe enters the resident map (K12) ----------------------------------------------------------------------------
KI_DIMS = (12, 140, 2000, 12)      # K, F, P, R: ten keyframes, the new one and a spare slot; 121 rows and the promotions
KEYFRAME_INSERT_KERNEL = "keyframe_insert_kernel"


def keyframe_insert_bytes(rows, with_point, mean_obs, promoted, removed_rows, deleted, P, K):
    """bytes one sequence moves, from the shapes: the frame's rows are read once and written into the table; a row with a point
    reads that point's type and count, moves its records one place back (52 bytes each, read and written) and writes the new
    front record; a promotion reads and writes one record and one table row; the leaving keyframe's rows are read and nulled,
    their points' counts read, one record list shifted (half of it on average) or, for a deleted point, two records read and
    one table row nulled; every point's type is read once for removeFrameCandidates; the lists and key points of K slots."""
    rec, row = 52, 48
    frame = rows * (16 + 24 + 4 + 1 + 4) + rows * row + 96 * 2 + 5 * 4 * 2
    refs = with_point * (8 + mean_obs * rec * 2 + rec + 4)
    promotions = promoted * (2 * rec + row + 8)
    walk = removed_rows * (4 + 4 + 4) + (removed_rows - deleted) * (mean_obs * rec) + deleted * (2 * 12 + 4 + 8)
    return frame + refs + promotions + walk + 4 * P + K * (4 * 2 + 4 + 20) + 5 * 4


def compiler_resources_keyframe_insert():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        from rpg_svo_amd.build import FLAGS
        r = subprocess.run([hipcc, *FLAGS, "-c", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rpg_svo_amd", "csrc"),
                            os.path.join(ROOT, "rpg_svo_amd", "csrc", "keyframe_insert.hip"), "-o", os.path.join(tmp, "ki.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    for blk in r.stderr.split("Function Name: ")[1:]:
        if KEYFRAME_INSERT_KERNEL in blk.split()[0]:
            g = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
            return {"vgprs": g("VGPRs"), "agprs": g("AGPRs"), "sgprs": g("TotalSGPRs"), "scratch_bytes_per_lane": g(r"ScratchSize \[bytes/lane\]"),
                    "occupancy_waves_per_simd": g(r"Occupancy \[waves/SIMD\]"), "lds_bytes_per_block": g(r"LDS Size \[bytes/block\]")}
    return "not measured"


def time_keyframe_insert(dev, n_seq, steps, warmup):
    """every timed call starts from the same map: the state is restored from a saved copy outside the events"""
    import numpy as np
    import torch
    import first_map_cases
    import keyframe_insert_cases as cases
    import keyframe_insert_checker as chk
    from rpg_svo_amd import sequence_map as sm
    cam = first_map_cases.camera(752, 480)
    K, F, P, R = KI_DIMS
    distinct = min(16, n_seq)
    seqs = [cases.random_seq(cam, KI_DIMS, ROWS, 9000 + k, KEYFRAMES, ROWS, ROWS, k % KEYFRAMES, n_cand=650, max_obs=2, n_pts=1200, match_cands=0.01)
            for k in range(distinct)]
    b = cases.batch("bench", cam, KI_DIMS, ROWS, seqs)
    reps = -(-n_seq // distinct)
    tile = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev).repeat(reps, *([1] * (v.ndim - 1)))
    state = {k: tile(b.state[k]) for k in chk.STATE}
    per_frame = lambda t: t[:n_seq * K].contiguous() if t.shape[0] == reps * distinct * K else t[:n_seq].contiguous()
    state = {k: per_frame(t) for k, t in state.items()}
    seq = torch.arange(n_seq, device=dev)
    state["obs_kf"] += ((seq - seq % distinct) * K).to(torch.int32)[:, None, None]      # frame = b * K + slot
    smap = sm.SequenceMap(n_seq, K, F, P, R, cam=cam, **state)
    saved = smap.clone()
    inp = {k: tile(b.inputs[0][k])[:n_seq].contiguous() for k in chk.INPUTS}
    out, times = None, []
    for i in range(warmup + steps):
        smap.copy_(saved)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = sm.insert_keyframe(smap, inp, out=out)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    times.sort()
    med = times[len(times) // 2]
    want = b.expect[0][1]
    assert all(np.array_equal(getattr(out, k)[:distinct].cpu().numpy(), want[k]) for k in chk.OUTPUTS), "the batch does not give the checker's outputs"
    with_point = float(np.mean([(b.expect[0][0]["ftr_point"][s * K + want["kf_new_slot"][s], :ROWS] >= 0).sum() for s in range(distinct)]))
    live = b.state["pt_type"] != 0
    removed_rows = float(np.mean([b.state["kf_n_fts"][s * K + b.state["kf_list"][s, b.inputs[0]["kf_remove"][s]]] for s in range(distinct)]))
    shape = dict(rows=ROWS, with_point=with_point, mean_obs=float(b.state["pt_n_obs"][live].mean()), promoted=float(want["n_promoted"].mean()),
                 removed_rows=removed_rows, deleted=float(want["n_points_deleted"].mean()), P=P, K=K)
    return {"sequences": n_seq, "keyframes": KEYFRAMES, "capacities_K_F_P_R": list(KI_DIMS), "points": float(live.sum(axis=1).mean()), "steps": steps,
            "call_ms_median": med, "call_ms_min": times[0], "call_ms_max": times[-1], "sequences_per_s": n_seq / (med * 1e-3), "per_sequence": shape,
            "status_ok_fraction": float((out.status == 0).float().mean().item()), "bytes_per_sequence": keyframe_insert_bytes(**shape)}


def traced_keyframe_insert_ms(args):
    """Kernel time of the replay shape from rocprofv3's kernel trace, in a run of its own."""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    out = tempfile.mkdtemp(prefix="keyframe_insert_trace_", dir=os.path.join(ROOT, "build"))
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "trace", "--", sys.executable,
           os.path.abspath(__file__), "--step", "keyframe_insert", "--traced-child", "--pairs", str(args.pairs)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
        return {"error": f"rocprofv3 exit {r.returncode}: {r.stderr[-400:]}"}
    for row in csv.DictReader(open(files[0])):
        if KEYFRAME_INSERT_KERNEL in row.get("Name", ""):
            return {"calls": int(row["Calls"]), "average_ms": float(row["AverageNs"]) * 1e-6, "min_ms": float(row["MinNs"]) * 1e-6,
                    "max_ms": float(row["MaxNs"]) * 1e-6}
    return {"error": "the kernel is not in the trace"}


def main_keyframe_insert(args):
    import torch
    out = args.out or os.path.join(ROOT, "profiles", "keyframe_insert_bench.json")
    if not torch.cuda.is_available():
        res = {"device": "not measured", "replay_batch": "not measured", "rocprofv3": "not measured",
               "compiler": "not measured" if args.no_compiler else compiler_resources_keyframe_insert(),
               "note": "no MI355X was available: nothing here is measured without one"}
    else:
        dev = torch.device("cuda:0")
        if args.traced_child:
            time_keyframe_insert(dev, args.pairs, 3, 1)
            return
        res = {"device": torch.cuda.get_device_name(0), "library": os.environ.get("SVO_HIP_LIB", "in-tree")}
        res["replay_batch"] = time_keyframe_insert(dev, args.pairs, args.steps, args.warmup)
        res["compiler"] = "not measured" if args.no_compiler else compiler_resources_keyframe_insert()
        res["rocprofv3"] = "not measured" if args.no_trace else traced_keyframe_insert_ms(args)
        kern = res["rocprofv3"].get("average_ms") if isinstance(res["rocprofv3"], dict) else None
        t_ms = kern if kern else res["replay_batch"]["call_ms_median"]
        nbytes = res["replay_batch"]["bytes_per_sequence"] * args.pairs
        res["hbm_bound"] = {"time_basis": "rocprofv3 kernel time" if kern else "device events", "time_ms": t_ms, "bytes": nbytes,
                            "peak_bytes_per_s": PEAK_HBM_BYTES, "least_ms_by_bytes": nbytes / PEAK_HBM_BYTES * 1e3,
                            "achieved_bytes_per_s": nbytes / (t_ms * 1e-3), "share_of_bound": nbytes / PEAK_HBM_BYTES * 1e3 / t_ms,
                            "frame_close_kernel_ms_same_batch": 0.082}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-compiler", action="store_true", help="skip the compile that reports registers, scratch and occupancy")
    ap.add_argument("--traced-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--step", choices=("homography", "first_map", "frame_close", "keyframe_insert"), default="homography", help="which step of the bootstrap to time")
    ap.add_argument("--out", default=None, help="default: profiles/<step>_bench.json")
    args = ap.parse_args()
    if args.step == "first_map":
        return main_first_map(args)
    if args.step == "frame_close":
        return main_frame_close(args)
    if args.step == "keyframe_insert":
        return main_keyframe_insert(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "homography_bench.json")
    import torch
    if not torch.cuda.is_available():
        res = {"device": "not measured", "single_pair": "not measured", "replay_batch": "not measured", "rocprofv3": "not measured",
               "compiler": "not measured" if args.no_compiler else compiler_resources(),
               "f64_ops_per_pair": operations(POINTS, 512, 10), "note": "no MI355X was available: nothing here is measured without one"}
    else:
        dev = torch.device("cuda:0")
        if args.traced_child:
            time_shape(dev, args.pairs, 3, 1)
            return
        res = {"device": torch.cuda.get_device_name(0), "library": os.environ.get("SVO_HIP_LIB", "in-tree")}
        res["single_pair"] = time_shape(dev, 1, max(args.steps, 10), 5)
        res["single_pair"]["note"] = "one workgroup on one CU: launch- and latency-bound"
        res["replay_batch"] = time_shape(dev, args.pairs, args.steps, args.warmup)
        res["compiler"] = "not measured" if args.no_compiler else compiler_resources()
        res["rocprofv3"] = "not measured" if args.no_trace else traced_kernel_ms(args)
        kern = res["rocprofv3"].get("average_ms") if isinstance(res["rocprofv3"], dict) else None
        t_ms = kern if kern else res["replay_batch"]["call_ms_median"]
        ops = res["replay_batch"]["f64_ops_per_pair"] * args.pairs
        res["f64_bound"] = {"time_basis": "rocprofv3 kernel time" if kern else "device events", "time_ms": t_ms, "f64_ops": ops,
                            "peak_f64_ops_per_s": PEAK_F64_OPS, "least_ms_by_operations": ops / PEAK_F64_OPS * 1e3,
                            "achieved_f64_ops_per_s": ops / (t_ms * 1e-3), "share_of_bound": ops / PEAK_F64_OPS * 1e3 / t_ms,
                            "klt_track_ms_same_batch": KLT_TRACK_MS, "share_of_klt_track": t_ms / KLT_TRACK_MS}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
