"""svo_hip_frame_close on the device, through the Python mirror (rpg_svo_amd.tracking.close_frame), on the cases of
tests/frame_close_cases.py -- the cases of tests/test_frame_close_emulated.py, here with the real LDS atomics and the real f64
division and square root -- against the sequential checker (tests/frame_close_checker.py).  Rule
(first_map_cases.compare_device): gates, quality, result, counts, indices, key points, valid and occupancy are equal; f64
outputs are expected equal and fail above 1e-14 relative (K10's bound for the same arithmetic).  Every test prints its largest
difference.  Outputs start poisoned.  Also: the same bits for identical sequences at different batch positions and for a
repeated call; the error codes through the mirror; one HIP graph of close_frame -> SparseImgAlign.run on its outputs,
replayed twice on poisoned buffers, with the bits of the eager run.

Measured on an MI355X: every output of all 34 batches has the checker's bits (largest relative difference 0); the graph
test's batch gives gates [0, 0, 3, 1] and K1 n_tracked [65, 27, 108, 34], eager and replayed alike, difference to the checker 0.
On the emulation every output has the checker's bits too."""
import numpy as np
import pytest
import torch

import frame_close_cases as cases
from first_map_cases import compare_device
from host_buffers import same_bits

pytestmark = pytest.mark.gpu


def poison(fc):
    for k in cases.out_shapes(1, 1, 1):
        t = getattr(fc, k)
        t.fill_(float("nan") if t.dtype == torch.float64 else 0x55)
    return fc


def run(dev, b, out=None, **override):
    from rpg_svo_amd import tracking as tr
    inp = {k: torch.from_numpy(v).to(dev) for k, v in cases.inputs(b).items()}
    cell_size, n_cols, n_rows = b.grid
    if out is None:
        out = poison(tr.frame_close_outputs(len(b.seqs), b.n_stride, n_cols * n_rows, dev))
    kw = dict(cell_size=cell_size, grid_n_cols=n_cols, grid_n_rows=n_rows, params=tr.frame_close_params(**b.params), out=out)
    kw.update(override)
    tr.close_frame(b.cam, *[inp[k] for k in cases.INPUTS], **kw)
    torch.cuda.synchronize()
    return {k: getattr(out, k).cpu().numpy() for k in cases.out_shapes(1, 1, 1)}


@pytest.mark.parametrize("name", cases.NAMES)
def test_frame_close_against_checker(gpu_device, name):
    b = cases.batches()[name]
    got = run(gpu_device, b)
    worst, _ = compare_device(got, b.expect, cases.DISCRETE, cases.CONTINUOUS, what=name)
    print(f"{name}: largest relative difference of an f64 output {worst:.2e}")


def test_identical_sequences_and_repeated_calls_give_the_same_bits(gpu_device):
    b = cases.batches()["every_exit"]
    one, two = run(gpu_device, b), run(gpu_device, b)
    for k in one:
        assert same_bits(one[k], two[k]), k
        for i, j in ((0, 5), (0, 15), (2, 7), (4, 9), (3, 13)):
            assert same_bits(one[k][i], one[k][j]), (k, i, j)


def test_limits_and_error_codes(gpu_device):
    from rpg_svo_amd import capi, tracking as tr
    b = cases.batches()["rows65"]
    cell_size, n_cols, n_rows = b.grid
    with pytest.raises(capi.SvoHipError, match="code -1"):
        run(gpu_device, b, cell_size=0)
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=gpu_device)
    i32 = torch.int32
    big, kfs = capi.FRAME_CLOSE_MAX_ROWS + 1, capi.FRAME_CLOSE_MAX_KFS + 1
    rows = lambda ns, nk: (z(1, dt=i32), z(1, ns, 2), z(1, ns, 3), z(1, ns, 3), z(1, ns, dt=torch.uint8), z(1, 12), z(1, 12), z(1, dt=i32),
                           z(1, dt=i32), z(1, dt=i32), z(1, nk, 12), z(1, nk, dt=i32))
    for ns, nk in ((big, 4), (8, kfs)):
        with pytest.raises(capi.SvoHipError, match="code -2"):
            tr.close_frame(b.cam, *rows(ns, nk), cell_size, n_cols, n_rows)
    # B == 0 touches nothing; a missing input is refused before anything is written
    import ctypes as C
    inp = [torch.from_numpy(v).to(gpu_device) for v in cases.inputs(b).values()]
    out = poison(tr.frame_close_outputs(len(b.seqs), b.n_stride, n_cols * n_rows, gpu_device))
    lib, cam, p = capi.load(), capi.camera(b.cam), tr.frame_close_params()
    o = capi.FrameCloseOut(*[getattr(out, k).data_ptr() for k in capi.FRAME_CLOSE_OUTPUTS])
    full = capi.FrameCloseIn(*[t.data_ptr() for t in inp])
    holed = capi.FrameCloseIn(*[None if k == 3 else t.data_ptr() for k, t in enumerate(inp)])
    call = lambda B, i: lib.svo_hip_frame_close(C.byref(cam), B, b.n_stride, b.kf_stride, C.byref(i), cell_size, n_cols, n_rows, n_cols * n_rows,
                                                C.byref(p), C.byref(o), None)
    assert call(0, full) == 0 and call(len(b.seqs), holed) == -1
    torch.cuda.synchronize()
    assert bool((out.gate == 0x55).all()) and bool(torch.isnan(out.xyz_ref).all()) and bool((out.occupancy == 0x55).all())


def test_a_graph_of_close_frame_and_k1_replays_the_eager_bits(gpu_device):
    """close_frame followed by SparseImgAlign.run on its xyz_ref / valid (and the frame's px as it is), on one side stream,
    captured once as a HIP graph and replayed twice on poisoned outputs: every output has the bits of the eager run."""
    import klt_scenes
    from rpg_svo_amd import tracking as tr
    from rpg_svo_amd.sparse_img_align import SparseImgAlign
    from test_klt_gpu import make_store
    dev = gpu_device
    cam = klt_scenes.small_camera()
    rng = np.random.default_rng(3)
    noise = rng.uniform(0, 255, (cam.height + 8, cam.width + 8))
    smooth = sum(noise[dy:dy + cam.height, dx:dx + cam.width] for dy in range(8) for dx in range(8)) / 64.0    # an 8 x 8 box filter
    smooth = (smooth - smooth.min()) / (smooth.max() - smooth.min()) * 255.0
    images = np.stack([smooth, np.roll(smooth, (1, 2), axis=(0, 1))]).astype(np.uint8)
    store = make_store(images, dev)
    seqs = [cases.make_seq(cam, 900 + k, 130, n, points=m, num_obs=a, num_obs_last=100) for k, (n, m, a) in
            enumerate(((121, "random", 90), (60, "alternating", 65), (130, "all", 30), (40, "all", 60)))]
    b = cases._batch("graph", seqs, 30)
    cell_size, n_cols, n_rows = b.grid
    inp = {k: torch.from_numpy(v).to(dev) for k, v in cases.inputs(b).items()}
    B = len(seqs)
    fc = tr.frame_close_outputs(B, b.n_stride, n_cols * n_rows, dev)
    sia = SparseImgAlign(4, 2)
    k1 = sia.alloc_result(B, dev)
    ref_slot, cur_slot = torch.zeros(B, dtype=torch.int32, device=dev), torch.ones(B, dtype=torch.int32, device=dev)
    prior = torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=torch.float64, device=dev).repeat(B, 1)
    n_rows_seq = torch.clamp(inp["n"], 0, b.n_stride)

    def chain():
        tr.close_frame(cam, *[inp[k] for k in cases.INPUTS], cell_size, n_cols, n_rows, out=fc)
        sia.run(store, cam, ref_slot, cur_slot, n_rows_seq, inp["px"], fc.xyz_ref, prior, valid=fc.valid, out=k1)

    def held():
        t = {k: getattr(fc, k) for k in cases.out_shapes(1, 1, 1)}
        t.update(k1_T=k1.T_cur_from_ref, k1_n_tracked=k1.n_tracked, k1_chi2=k1.chi2)
        return t

    def poison_all():
        for v in held().values():
            v.fill_(float("nan") if v.is_floating_point() else 0x55)

    poison_all()
    chain()
    torch.cuda.synchronize()
    eager = {k: v.cpu().numpy().copy() for k, v in held().items()}
    want = cases.chk.frame_close(cam, cases.inputs(b), *b.grid)
    worst, _ = compare_device(eager, want, cases.DISCRETE, cases.CONTINUOUS, what="graph")
    print(f"eager: gate {eager['gate'].tolist()}, result {eager['result'].tolist()}, K1 n_tracked {eager['k1_n_tracked'].tolist()}, largest "
          f"relative difference to the checker {worst:.2e}")
    assert list(eager["gate"]) == [0, 0, 3, 1] and eager["k1_n_tracked"][0] > 0

    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        chain()
    for _ in range(2):
        poison_all()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for k, v in held().items():
            assert same_bits(v.cpu().numpy(), eager[k]), k
