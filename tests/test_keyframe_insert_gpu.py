"""svo_hip_keyframe_insert on the device, through the Python mirror (rpg_svo_amd.sequence_map.insert_keyframe), on the cases of
tests/keyframe_insert_cases.py -- the cases of tests/test_keyframe_insert_emulated.py, here with the real LDS atomics, barriers
and global memory -- against the list-based checker (tests/keyframe_insert_checker.py): every array of the state and every
output byte for byte after every call (the results are integers and copies of input doubles: no tolerance).  Outputs start
poisoned.  Also: repeated calls from the same start give the same bytes; a captured graph of "restore the state from a saved
copy, then insert_keyframe" (one stream, no parallel branches), replayed twice on poisoned outputs, gives the eager bytes; the
error codes through the mirror.

Measured on an MI355X: all 37 batches have the checker's bytes; the graph's two replays have the eager run's."""
import numpy as np
import pytest
import torch

import keyframe_insert_cases as cases
import keyframe_insert_checker as chk
from host_buffers import same_bits

pytestmark = pytest.mark.gpu


def upload(b, dev):
    from rpg_svo_amd import sequence_map as sm
    smap = sm.SequenceMap(b.B, *b.dims, cam=b.cam, **{k: torch.from_numpy(np.ascontiguousarray(b.state[k])).to(dev) for k in chk.STATE})
    calls = [{k: torch.from_numpy(np.ascontiguousarray(inp[k])).to(dev) for k in chk.INPUTS} for inp in b.inputs]
    return smap, calls


def poisoned(B, dev):
    from rpg_svo_amd import sequence_map as sm
    out = sm.keyframe_insert_outputs(B, dev)
    for k in chk.OUTPUTS:
        getattr(out, k).fill_(0x55555555)
    return out


def download(smap, out):
    torch.cuda.synchronize()
    return {k: getattr(smap, k).cpu().numpy() for k in chk.STATE}, {k: getattr(out, k).cpu().numpy() for k in chk.OUTPUTS}


def assert_same(state, out, want_state, want_out, what):
    for k in chk.OUTPUTS:
        assert same_bits(out[k], want_out[k]), (what, k, out[k].tolist(), want_out[k].tolist())
    for k in chk.STATE:
        assert same_bits(state[k], want_state[k]), (what, k)


@pytest.mark.parametrize("name", cases.NAMES)
def test_keyframe_insert_against_checker(gpu_device, name):
    from rpg_svo_amd import sequence_map as sm
    b = cases.batches()[name]
    smap, calls = upload(b, gpu_device)
    for c, (fld, (want_state, want_out)) in enumerate(zip(calls, b.expect)):
        out = sm.insert_keyframe(smap, fld, out=poisoned(b.B, gpu_device))
        assert_same(*download(smap, out), want_state, want_out, (name, c))


def test_repeated_calls_from_the_same_start_give_the_same_bytes(gpu_device):
    from rpg_svo_amd import sequence_map as sm
    for name in ("few_records_47x33", "rows_255_256_257"):
        b = cases.batches()[name]
        runs = []
        for _ in range(3):
            smap, calls = upload(b, gpu_device)
            runs.append(download(smap, sm.insert_keyframe(smap, calls[0], out=poisoned(b.B, gpu_device))))
        for state, out in runs[1:]:
            assert_same(state, out, *runs[0], name)


def test_a_graph_of_restore_and_insert_replays_the_eager_bytes(gpu_device):
    """copy the saved state over the live one, then insert_keyframe, on one side stream: captured once, replayed twice on
    poisoned outputs and a state the previous replay has changed"""
    from rpg_svo_amd import sequence_map as sm
    dev = gpu_device
    b = cases.batches()["few_records_160x120"]
    smap, calls = upload(b, dev)
    saved = smap.clone()
    out = poisoned(b.B, dev)

    def chain():
        smap.copy_(saved)
        sm.insert_keyframe(smap, calls[0], out=out)

    chain()
    eager = download(smap, out)
    assert_same(*eager, *b.expect[0], "eager")
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        chain()
    for _ in range(2):
        for k in chk.OUTPUTS:
            getattr(out, k).fill_(0x55555555)
        torch.cuda.synchronize()
        graph.replay()
        assert_same(*download(smap, out), *eager, "replay")


def test_limits_and_error_codes(gpu_device):
    from rpg_svo_amd import capi, sequence_map as sm
    dev = gpu_device
    b = cases.batches()["overflow"]
    smap, calls = upload(b, dev)
    out = poisoned(b.B, dev)
    wide = {k: (torch.zeros(b.B, 1025, *v.shape[2:], dtype=v.dtype, device=dev) if v.dim() >= 2 and v.shape[1] == b.n_stride else v) for k, v in calls[0].items()}
    with pytest.raises(capi.SvoHipError, match="code -2"):
        sm.insert_keyframe(smap, wide, out=out)
    import ctypes as C
    m, cam = smap.struct(), capi.camera(b.cam)
    i = capi.KeyframeInsertIn(*[calls[0][k].data_ptr() for k in capi.KEYFRAME_INSERT_INPUTS])
    holed = capi.KeyframeInsertIn(*[None if k == "ftr_point" else calls[0][k].data_ptr() for k in capi.KEYFRAME_INSERT_INPUTS])
    o = capi.KeyframeInsertOut(*[getattr(out, k).data_ptr() for k in capi.KEYFRAME_INSERT_OUTPUTS])
    lib = capi.load()
    assert lib.svo_hip_keyframe_insert(C.byref(cam), 0, b.n_stride, C.byref(m), C.byref(i), C.byref(o), None) == 0
    assert lib.svo_hip_keyframe_insert(C.byref(cam), b.B, b.n_stride, C.byref(m), C.byref(holed), C.byref(o), None) == -1
    assert lib.svo_hip_keyframe_insert(C.byref(cam), b.B, b.n_stride, None, C.byref(i), C.byref(o), None) == -1
    state, got = download(smap, out)
    assert all((got[k] == 0x55555555).all() for k in chk.OUTPUTS)
    for k in chk.STATE:
        assert same_bits(state[k], b.state[k]), k
