"""TEST INFRASTRUCTURE.  The named K1 problems of the width tests (tests/test_sparse_align_width_gpu.py, and the single-step and
shape cases of the emulated tests): every case is a function returning (helpers.Batch, (max_level, min_level, n_iter)), built
from seeded numpy draws and rpg_svo_amd.synth alone (no GPU, no oracle), so that the child process that runs the reference-width library
(tests/k1_width_child.py) and the parent that holds the oracle build the same inputs, bit for bit.  None is the workload's
size."""
import numpy as np
import torch

from helpers import camera_models, make_batch, tile_batch
from rpg_svo_amd import se3, synth

# (w, h, patches, pyramid levels, min_level, max_level): every workgroup size of sia_kernel -- 64, 128, 256, 512 (twice) and
# 1024 lanes; the last one is also the frame svo_hip_sparse_align splits over four workgroups
SHAPES = [(160, 120, 9, 3, 0, 2), (200, 150, 65, 3, 1, 2), (322, 242, 129, 4, 0, 3), (328, 248, 257, 4, 2, 3),
          (336, 256, 300, 3, 0, 2), (400, 300, 520, 4, 0, 3)]
SHAPE_IDS = [f"{w}x{h}_n{n}" for w, h, n, *_ in SHAPES]


def shape_case(w, h, n, levels, lo, hi):
    """three frames of an odd-sized image, the middle one ragged: a third of the patches, or -- for the 520-patch frame, so that
    it stays a frame of more than 512 -- 513 of them"""
    if n == 520:
        seq = synth.make_sequence(4, 520, cam=synth.Camera(400, 300, 240, 240, 200, 150), seed=520, margin=12, cell=10)
    else:
        cam = synth.Camera(w, h, w * 0.6, w * 0.6, w / 2.0, h / 2.0)
        seq = synth.make_sequence(4, n, cam=cam, seed=n, margin=12, cell=max(8, int((w * h / n) ** 0.5 * 0.7)))
    b = make_batch(seq, [(0, 1), (1, 2), (2, 3)], levels)
    b.n[1] = 513 if n == 520 else max(6, n // 3)
    return b, (hi, lo, 30)


_seqs = {}


def _seq(*a, **kw):
    key = (a, tuple(sorted((k, repr(v)) for k, v in kw.items())))
    if key not in _seqs:
        _seqs[key] = synth.make_sequence(*a, **kw)
    return _seqs[key]


def _seq_vga():
    return _seq(17, 200)


def vga16():
    """the benchmark's instantiation, sia_kernel<256, true, false>: VGA, 200 patches, levels 3 -> 0"""
    return make_batch(_seq_vga(), [(i, i + 1) for i in range(16)], 4), (3, 0, 30)


def _distorted(kind, hi, lo):
    seq = _seq(6, 120, cam=camera_models()[kind], seed=9, margin=56, cell=40)
    return make_batch(seq, [(i, i + 1) for i in range(5)], 5), (hi, lo, 30)


def atan_520():
    """the distorted instantiation of the frame split over four workgroups (and of the 1024-lane workgroup)"""
    seq = _seq(4, 520, cam=camera_models()["atan"], seed=521, margin=28, cell=16)
    b = make_batch(seq, [(0, 1), (1, 2), (2, 3)], 4)
    b.n[1] = 513
    return b, (3, 0, 30)


def ragged():
    """tests/test_sparse_align_gpu.py::test_ragged_and_missing_points"""
    rng = np.random.default_rng(11)
    pairs = [(0, 1), (3, 4), (5, 6), (8, 9), (9, 10), (12, 11), (13, 14)]
    hp = (rng.random((7, 200)) > 0.3).astype(np.uint8)
    hp[0] = 1
    hp[6] = 1
    return make_batch(_seq_vga(), pairs, 4, n_valid=[200, 12, 64, 65, 137, 0, 1], has_point=hp), (3, 0, 30)


def _border_seq():
    if "border" not in _seqs:
        seq = synth.make_sequence(5, 200, seed=3)
        rng = np.random.default_rng(3)
        for i in range(5):   # 40 features per frame into the 3..30 px band next to a border
            k = rng.choice(200, 40, replace=False)
            side = rng.integers(0, 4, size=40)
            off = rng.uniform(3.0, 30.0, size=40)
            u, v = seq.px[i, k, 0].numpy().copy(), seq.px[i, k, 1].numpy().copy()
            u[side == 0] = off[side == 0]
            u[side == 1] = 639.0 - off[side == 1]
            v[side == 2] = off[side == 2]
            v[side == 3] = 479.0 - off[side == 3]
            seq.px[i, k, 0] = torch.from_numpy(u)
            seq.px[i, k, 1] = torch.from_numpy(v)
        seq.f, seq.pos = synth.features_3d(seq.T_f_w, seq.cam, seq.px)
        _seqs["border"] = seq
    return _seqs["border"]


def _border(lo):
    return make_batch(_border_seq(), [(0, 1), (1, 2), (2, 3), (3, 4), (4, 3)], 4), (3, lo, 30)


def outside():
    """a prior so wrong that nothing of the first frame projects into the image"""
    b = make_batch(_seq_vga(), [(0, 1), (2, 3)], 4)
    b.T_cur_w = se3.mul(se3.exp(np.array([[50.0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0.0, 0]])), b.T_cur_w)
    return b, (3, 0, 30)


def _itercap(n_iter):
    return make_batch(_seq_vga(), [(0, 1), (4, 5)], 4), (3, 0, n_iter)


def sample256():
    """256 different problems (16 pairs x 16 priors) for the share of identical per-level iteration sequences"""
    return make_batch(_seq_vga(), [(i, i + 1) for i in range(16)] * 16, 4, prior="ref", prior_noise=2e-3, seed=5), (3, 0, 30)


STEP_PRIOR_NOISE = 5e-3


def single_step(level):
    """ONE Gauss-Newton step at one level from a prior 5e-3 off in rotation and translation alike: nothing corrects a
    first-order error of SE3::exp or of a product afterwards"""
    seq = _seq(13, 200)
    b = make_batch(seq, [(i, i + 1) for i in range(12)], 4, prior="ref", prior_noise=STEP_PRIOR_NOISE, seed=17)
    return b, (level, level, 1)


def wave1024():
    """32 pairs x 60 patches, tiled to B = 1024: svo_hip_sparse_align gives such a batch to the wave-per-frame kernel"""
    seq = _seq(33, 60, seed=23)
    b = make_batch(seq, [(i, i + 1) for i in range(32)], 4)
    b.n[3] = 53
    b.has_point[5, ::3] = 0
    return tile_batch(b, 32), (3, 0, 30)


CASES = {f"shape_{i}": (lambda s=s: shape_case(*s)) for i, s in zip(SHAPE_IDS, SHAPES)}
CASES.update({
    "vga16": vga16,
    "radtan_4to2": lambda: _distorted("radtan", 4, 2), "radtan_3to0": lambda: _distorted("radtan", 3, 0),
    "atan_4to2": lambda: _distorted("atan", 4, 2), "atan_3to0": lambda: _distorted("atan", 3, 0),
    "atan_520": atan_520,
    "ragged": ragged, "border_3to0": lambda: _border(0), "border_3to2": lambda: _border(2), "outside": outside,
    "itercap_0": lambda: _itercap(0), "itercap_1": lambda: _itercap(1), "itercap_2": lambda: _itercap(2),
    "sample256": sample256,
    "step_level3": lambda: single_step(3), "step_level0": lambda: single_step(0),
    "wave1024": wave1024,
})
# cases that run through svo_hip_sparse_align_workgroup as well (kernel="workgroup": the 1024-lane workgroup where "auto" splits)
WORKGROUP_TOO = ("shape_400x300_n520", "atan_520")
# the case the child runs twice (determinism)
TWICE = "vga16"
