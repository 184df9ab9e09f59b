"""TEST INFRASTRUCTURE.  The device backend of the K1 tests: a case of tests/k1_cases.py through helpers.run_hip on the library
this process has bound (rpg_svo_amd.capi binds one per process: the default library, or in tests/k1_width_child.py the one
SVO_HIP_LIB names), tiled as the case says -- svo_hip_sparse_align gives batches of >= 1024 frames with <= 192 patches to the
wave-per-frame kernel.  kernel="workgroup" keeps every frame on one workgroup (svo_hip_sparse_align_workgroup)."""
import k1_cases
from helpers import run_hip, tile_batch


def answer(T_cur_w, out):
    """helpers.run_hip's poses and tensors as a K1Answer"""
    f = lambda a: a.cpu().numpy()
    return k1_cases.K1Answer(T_cur_w, f(out.iters), f(out.n_tracked), f(out.status), f(out.H).reshape(len(T_cur_w), 36), f(out.chi2))


def run_batch(b, schedule, kernel="auto"):
    T, out, _ = run_hip(b, *schedule, kernel=kernel)
    return answer(T, out)


def run(case, schedule, kernel="auto"):
    b = case.batch
    return run_batch(tile_batch(b, case.tile) if case.tile > 1 else b, schedule, kernel)
