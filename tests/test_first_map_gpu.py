"""svo_hip_first_map and svo_hip_initialize_seeds on the device, through the Python mirror
(rpg_svo_amd.initialization.first_map, rpg_svo_amd.tracking.DepthFilter.initialize_seeds), on the cases of
tests/first_map_cases.py -- the cases of tests/test_first_map_emulated.py, here with the real LDS atomics and the real f64
division and square root -- against the sequential checker (tests/first_map_checker.py).  Rule (first_map_cases.compare_device):
counts, indices, key points, occupancy, batch_id, level and type are equal; f64 outputs are expected equal and fail above
1e-14 relative; the f32 seed fields fail above 1 ulp.  Every test prints its largest differences.  Outputs start poisoned.
Also: the same bits for identical sequences at different batch positions and for a repeated call; the error codes through
the mirror; one HIP graph of K8 -> K9 -> first map -> detect -> seeds, replayed twice, with the bits of the eager run.

Measured on an MI355X: every output of all 32 first-map batches and all 10 seed cases has the checker's bits (largest
relative difference 0, 0 ulp); the graph test's scene gives result [SUCCESS, FAILURE], 263 / 0 points and 130 / 0 seeds, eager
and replayed alike.  On the emulation every output has the checker's bits too."""
import numpy as np
import pytest
import torch

import first_map_cases as cases
from host_buffers import same_bits

pytestmark = pytest.mark.gpu


def poisoned(fm):
    for k in cases.out_shapes(1, 1, 1):
        t = getattr(fm, k)
        t.fill_(float("nan") if t.dtype == torch.float64 else 0x55)
    return fm


def run_first_map(dev, b, out=None):
    from rpg_svo_amd import initialization as init
    inp = {k: torch.from_numpy(v).to(dev) for k, v in cases.inputs(b).items()}
    cell_size, n_cols, n_rows = b.grid
    if out is None:
        out = poisoned(init.first_map_outputs(len(b.seqs), b.n_pts, n_cols * n_rows, dev))
    init.first_map(b.cam, *[inp[k] for k in cases.INPUTS], cell_size, n_cols, n_rows, out)
    torch.cuda.synchronize()
    return {k: getattr(out, k).cpu().numpy() for k in cases.out_shapes(1, 1, 1)}


def run_seeds(dev, c, stride, batch_id):
    from rpg_svo_amd.tracking import DepthFilter, FeatureSet, SeedSet
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    full = lambda dt, *tail: torch.full((c.n_frames, stride, *tail), float("nan") if dt.is_floating_point else 0x55, dtype=dt, device=dev)
    ftr = FeatureSet(full(torch.int32), full(torch.int32), full(torch.float64, 2), full(torch.float64, 3), full(torch.uint8), full(torch.float64, 2))
    seeds = SeedSet(*[full(torch.float32) for _ in range(5)], full(torch.int32))
    n_seeds = torch.full((c.n_frames,), 0x55, dtype=torch.int32, device=dev)
    DepthFilter.initialize_seeds(c.cam, t(c.xy), t(c.level), t(c.score), c.threshold, t(c.frame_index), t(c.depth_mean), t(c.depth_min),
                                 batch_id, seed_stride=stride, out=(ftr, seeds, n_seeds))
    torch.cuda.synchronize()
    got = dict(n_seeds=n_seeds, frame=ftr.frame, level=ftr.level, type=ftr.type, px=ftr.px, f=ftr.f, grad=ftr.grad, a=seeds.a, b=seeds.b,
               mu=seeds.mu, z_range=seeds.z_range, sigma2=seeds.sigma2, batch_id=seeds.batch_id)
    return {k: v.cpu().numpy() for k, v in got.items()}


@pytest.mark.parametrize("name", cases.NAMES)
def test_first_map_against_checker(gpu_device, name):
    b = cases.batches()[name]
    got = run_first_map(gpu_device, b)
    worst, _ = cases.compare_device(got, b.expect, cases.DISCRETE, cases.CONTINUOUS, what=name)
    print(f"{name}: largest relative difference of an f64 output {worst:.2e}")


@pytest.mark.parametrize("name", cases.SEED_NAMES)
def test_seeds_against_checker(gpu_device, name):
    c, stride, batch_id = cases.seed_cases()[name]
    got = run_seeds(gpu_device, c, stride, batch_id)
    worst, ulps = cases.compare_device(got, c.expect, cases.SEED_DISCRETE, cases.SEED_F64, cases.SEED_F32, what=name)
    cases.check_seed_rule(c, got)     # (no record for a level -1 cell, whatever its score: thresholds 20.1 and 0.1 round up in float)
    print(f"{name}: largest relative difference of an f64 output {worst:.2e}, of an f32 seed field {ulps} ulp")


def test_identical_sequences_and_repeated_calls_give_the_same_bits(gpu_device):
    for name, twins in (("failed_between", (0, 2, 5)), ("sixteen", (0, 3, 15))):
        b = cases.batches()[name]
        one, two = run_first_map(gpu_device, b), run_first_map(gpu_device, b)
        for k in one:
            assert same_bits(one[k], two[k]), k
            for j in twins[1:]:
                assert same_bits(one[k][twins[0]], one[k][j]), (k, j)


def test_limits_and_error_codes(gpu_device):
    from rpg_svo_amd import capi, initialization as init
    from rpg_svo_amd.tracking import DepthFilter
    b = cases.batches()["n63"]
    inp = [torch.from_numpy(v).to(gpu_device) for v in cases.inputs(b).values()]
    cell_size, n_cols, n_rows = b.grid
    with pytest.raises(capi.SvoHipError, match="code -1"):
        init.first_map(b.cam, *inp, 0, n_cols, n_rows)
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=gpu_device)
    big = capi.FIRST_MAP_MAX_PTS + 1
    many = (z(1, dt=torch.int32), z(1, big, dt=torch.uint8), z(1, big, 3), z(1, big, 2, dt=torch.float32), z(1, big, 2, dt=torch.float32),
            z(1, big, 3), z(1, big, 3), z(1, 12), z(1, 12))
    with pytest.raises(capi.SvoHipError, match="code -2"):
        init.first_map(b.cam, *many, cell_size, n_cols, n_rows)
    out = poisoned(init.first_map_outputs(len(b.seqs), b.n_pts, n_cols * n_rows + 1, gpu_device))   # cells != cols * rows
    lib, cam = capi.load(), capi.camera(b.cam)
    import ctypes as C
    o = capi.FirstMapOut(*[getattr(out, k).data_ptr() for k in capi.FIRST_MAP_OUTPUTS])
    args = [t.data_ptr() for t in inp]
    assert lib.svo_hip_first_map(C.byref(cam), len(b.seqs), b.n_pts, *args, cell_size, n_cols, n_rows, n_cols * n_rows + 1, C.byref(o), None) == -1
    assert lib.svo_hip_first_map(C.byref(cam), len(b.seqs), b.n_pts, None, *args[1:], cell_size, n_cols, n_rows, n_cols * n_rows, C.byref(o), None) == -1
    assert lib.svo_hip_first_map(C.byref(cam), 0, b.n_pts, *args, cell_size, n_cols, n_rows, n_cols * n_rows, C.byref(o), None) == 0   # a no-op
    torch.cuda.synchronize()
    assert bool((out.n_points == 0x55).all()) and bool(torch.isnan(out.pos).all())
    c, stride, batch_id = cases.seed_cases()["wide_stride"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    with pytest.raises(capi.SvoHipError, match="code -1"):
        DepthFilter.initialize_seeds(c.cam, t(c.xy), t(c.level), t(c.score), c.threshold, t(c.frame_index), t(c.depth_mean), t(c.depth_min),
                                     batch_id, seed_stride=c.n_cells - 1)


def test_a_graph_of_the_whole_bootstrap_replays_the_eager_bits(gpu_device):
    """K8 -> K9 -> first map -> detect -> seeds of two sequences (the rendered scene of tests/test_bootstrap_to_tracking_gpu.py
    at the frame that gives SUCCESS, and a flat image that fails), captured once as a HIP graph on a side stream and
    replayed twice on reused, poisoned buffers from the tracker state before that frame: every output has the bits of
    the eager run."""
    from rpg_svo_amd.initialization import InitResult
    from test_bootstrap_to_tracking_gpu import bootstrap
    s, store, slots, init, k, before = bootstrap(gpu_device)
    second = slots(k)

    def tensors(fm):
        t = {n: getattr(fm, n) for n in cases.out_shapes(1, 1, 1)}
        t.update(n_seeds=fm.n_seeds, seed_px=fm.seed_ftr.px, seed_f=fm.seed_ftr.f, seed_level=fm.seed_ftr.level, mu=fm.seeds.mu,
                 sigma2=fm.seeds.sigma2, batch_id=fm.seeds.batch_id, result=init.result, T_cur_w=init.out["T_cur_w"], point_w=init.out["point_w"])
        return t

    def restore():
        init.px_cur.copy_(before[0])
        init.status.copy_(before[1])

    def chain(out=None):
        init.add_second_frame(store, second)
        return init.first_map(store, second, batch_id=1, out=out)

    restore()
    fm = chain()
    torch.cuda.synchronize()
    eager = {n: v.cpu().numpy().copy() for n, v in tensors(fm).items()}
    print(f"eager: result {eager['result'].tolist()}, n_points {eager['n_points'].tolist()}, n_seeds {eager['n_seeds'].tolist()}")
    assert list(eager["result"]) == [InitResult.SUCCESS, InitResult.FAILURE]
    assert eager["n_points"][0] >= 40 and eager["n_points"][1] == 0 and eager["n_seeds"][0] > 0

    restore()
    side = torch.cuda.Stream(device=gpu_device)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        fm = chain(out=fm)
    held = tensors(fm)
    for _ in range(2):
        restore()
        for v in held.values():
            v.fill_(float("nan") if v.is_floating_point() else 0x55)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for n, v in held.items():
            assert same_bits(v.cpu().numpy(), eager[n]), n
