"""TEST INFRASTRUCTURE.  The emulated backend of the K1 tests: a case of tests/k1_cases.py through svo_hip_sparse_align of the
host-emulated library (tests/emu_build.py) -- sia_kernel with its LDS tiles, wave reductions, the two-wave solve and its
barriers on the CPU -- or, kernel="wave", through the test-only entry of the wave-per-frame kernel (svo_hip_sparse_align gives it
batches of >= 1024 frames only).  K1 has two widths: the default build and the reference-width one (-DSIA_F64_PARTIALS)."""
import ctypes as C

import numpy as np

import k1_cases
from helpers import marshal_problem
from host_buffers import ptr
from rpg_svo_amd import capi, se3

K1_BUILDS = (0, 2)   # indices into emu_build.BUILDS: the default and the reference-width (SIA_F64_PARTIALS) build of sparse_align.hip
K1_BUILD_IDS = ["default", "reference_width"]
ENTRIES = {"auto": "svo_hip_sparse_align", "wave": "emu_sparse_align_wave"}


def run_emulated(emu, b, max_level, min_level, n_iter=30, entry="svo_hip_sparse_align"):
    """a helpers.Batch through an entry of the emulated library `emu` -> K1Answer"""
    imgs = np.ascontiguousarray(b.images)
    n, h, w = imgs.shape
    layout = capi.pyr_layout(w, h, b.n_levels)
    store = np.zeros(capi.pyr_store_bytes(layout, n), np.uint8)
    assert emu.svo_hip_pyramid_build_tiled(C.byref(layout), ptr(store), 0, n, ptr(imgs), C.c_longlong(h * w), w, capi.HALFSAMPLE_AUTO, 0, None) == 0
    T_cr, xyz = marshal_problem(b.T_ref_w, b.T_cur_w, b.f, b.pos)
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
    ref_slot, cur_slot, nn = c(b.ref_slot, np.int32), c(b.cur_slot, np.int32), c(b.n, np.int32)
    px, xyz, T_in, valid = c(b.px, np.float64), c(xyz, np.float64), c(T_cr, np.float64), c(b.has_point, np.uint8)
    B, ns = px.shape[0], px.shape[1]
    d = tuple(getattr(b.cam, "d", (0.0,) * 5))
    P = capi.SiaParams(b.cam.fx, b.cam.fy, b.cam.cx, b.cam.cy, max_level, min_level, n_iter, int(getattr(b.cam, "model", 0)), 1e-6,
                       (C.c_double * 5)(*d))
    T_out, H = np.zeros((B, 12)), np.zeros((B, 36))
    n_tracked, iters = np.zeros(B, np.int32), np.zeros((B, capi.MAX_LEVELS), np.int32)
    chi2, status = np.zeros(B), np.zeros(B, np.int32)
    rc = getattr(emu, entry)(C.byref(layout), ptr(store), B, ptr(ref_slot), ptr(cur_slot), ptr(nn), ns, ptr(px), ptr(xyz), ptr(valid),
                             C.byref(P), ptr(T_in), ptr(T_out), ptr(H), ptr(n_tracked), ptr(iters), ptr(chi2), ptr(status), None)
    assert rc == 0, rc
    return k1_cases.K1Answer(se3.mul(T_out, b.T_ref_w), iters, n_tracked, status, H, chi2)


class Emulated:
    """one build of the emulated library as a backend: run(case, schedule, kernel) -> K1Answer on the leading frames the table
    of tests/k1_cases.py gives this backend"""

    def __init__(self, build_index):
        from emu_build import BUILDS, build_emulated
        self.lib = build_emulated(BUILDS[build_index])
        self.name = {0: k1_cases.EMU, 2: k1_cases.EMU_REF}[build_index]

    def backend(self, kernel="auto"):
        return k1_cases.EMU_WAVE if kernel == "wave" else self.name

    def run(self, case, schedule, kernel="auto"):
        frames = k1_cases.pair(case.name, self.backend(kernel), schedule).frames
        return run_emulated(self.lib, k1_cases.head(case.batch, frames), *schedule, entry=ENTRIES[kernel])
