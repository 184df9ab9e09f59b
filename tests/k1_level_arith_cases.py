"""TEST INFRASTRUCTURE.  The K1 problems of tests/test_k1_level_arith_emulated.py and tests/test_k1_level_arith_gpu.py: small
frames chosen for the per-level arithmetic of csrc/sia_common.h (the factored patch Hessian with its membership mask, the
packed template) -- every workgroup size up to 256 lanes at its edges, patches that are outside the reference image at coarse
levels only, patches that leave the current image during a level, frames with holes, a frame of more than 512 patches, the
wave-per-frame kernel's two patch layouts.  Each case is (helpers.Batch, (max_level, min_level, n_iter)), built from seeded
draws; the oracle's answer to a case is computed once per session (reference())."""
import numpy as np

import k1_width_cases
from helpers import camera_models, make_batch, run_oracle
from rpg_svo_amd import se3, synth

_QVGA = synth.Camera(320, 240, 200.0, 200.0, 160.0, 120.0)


def _qvga(n, cell):
    return k1_width_cases._seq(4, n, cam=_QVGA, seed=n, margin=12, cell=cell)


def counts_64():
    """64-lane workgroups: 1, 63 and 64 patches"""
    return make_batch(_qvga(64, 20), [(0, 1), (1, 2), (2, 3)], 3, n_valid=[1, 63, 64]), (2, 0, 30)


def counts_128():
    """128-lane workgroups: 65 and 128 patches"""
    return make_batch(_qvga(128, 14), [(0, 1), (1, 2)], 3, n_valid=[65, 128]), (2, 0, 30)


def counts_256():
    """256-lane workgroups (the benchmark's instantiation, the packed template): 200 and 256 patches"""
    return make_batch(_qvga(256, 10), [(0, 1), (1, 2)], 3, n_valid=[200, 256]), (2, 0, 30)


def holes():
    """has_point holes: three of ten patches have no point, in a full and in a ragged frame"""
    rng = np.random.default_rng(41)
    hp = (rng.random((2, 256)) > 0.3).astype(np.uint8)
    return make_batch(_qvga(256, 10), [(1, 2), (2, 3)], 3, n_valid=[256, 181], has_point=hp), (2, 0, 30)


def coarse_border():
    """VGA, 40 of 200 patches 3 .. 30 px from a border: within 3 px of it at level 3 (inb false, S = 0 there) and inside at
    level 0"""
    b = make_batch(k1_width_cases._border_seq(), [(0, 1), (2, 3)], 4)
    lvl3 = np.floor(b.px / 8.0)
    out3 = (lvl3[..., 0] < 3) | (lvl3[..., 1] < 3) | (lvl3[..., 0] + 3 >= 80) | (lvl3[..., 1] + 3 >= 60)
    lvl0 = np.floor(b.px)
    out0 = (lvl0[..., 0] < 3) | (lvl0[..., 1] < 3) | (lvl0[..., 0] + 3 >= 640) | (lvl0[..., 1] + 3 >= 480)
    assert out3.sum(axis=1).min() >= 10 and not out0.any()
    return b, (3, 0, 30)


def _inside_cur(b, T_cur_w, level):
    """[B, N]: does the patch project at least 3 px inside the current image at `level` under pose T_cur_w"""
    R, t = se3.split(T_cur_w)
    p = np.einsum("bij,bnj->bni", R, b.pos) + t[:, None, :]
    s = 1.0 / (1 << level)
    u = np.floor((b.cam.fx * p[..., 0] / p[..., 2] + b.cam.cx) * s)
    v = np.floor((b.cam.fy * p[..., 1] / p[..., 2] + b.cam.cy) * s)
    w, h = b.cam.width >> level, b.cam.height >> level
    return (u - 3 >= 0) & (v - 3 >= 0) & (u + 3 < w) & (v + 3 < h)


def leaving():
    """the border frames from a prior 4e-3 off: patches that are inside the current image at the first evaluation of a level
    and outside at the pose the level converges to (or the other way round) -- membership changes after the first iteration
    and H is rebuilt with those patches masked"""
    b = make_batch(k1_width_cases._border_seq(), [(0, 1), (2, 3)], 4, prior_noise=4e-3, seed=29)
    moved = sum((_inside_cur(b, b.T_cur_w, l) != _inside_cur(b, b.T_gt_w, l)).sum() for l in (3, 2))
    assert moved >= 2, moved
    return b, (3, 0, 30)


def frame_600():
    """one frame of 600 patches: the 1024-lane workgroup; on the device the frame split over four workgroups"""
    seq = k1_width_cases._seq(2, 600, cam=synth.Camera(400, 300, 240, 240, 200, 150), seed=600, margin=12, cell=9)
    return make_batch(seq, [(0, 1)], 3), (2, 0, 30)


def wave(n_patches):
    """the wave-per-frame kernel: one (60) and three (190) patches per lane, a ragged frame, a frame with holes"""
    seq = k1_width_cases._seq(5, n_patches, seed=23)
    b = make_batch(seq, [(i, i + 1) for i in range(4)], 4)
    b.n[1] = n_patches - 7
    b.has_point[2, ::3] = 0
    return b, (3, 0, 30)


def distorted(kind, n):
    """a radtan / atan camera of the reference's launch files: the DIST instantiations, 64 or 200 patches"""
    seq = k1_width_cases._seq(3, n, cam=camera_models()[kind], seed=9 + n, margin=56, cell=40 if n <= 64 else 24)
    return make_batch(seq, [(0, 1), (1, 2)], 5), (4, 2, 30)


def self_aligned():
    """current image = reference image, identity prior: every residual is exactly zero when the template and the warped patch
    round alike"""
    return make_batch(_qvga(256, 10), [(0, 0), (2, 2)], 3, n_valid=[256, 200]), (2, 0, 30)


WORKGROUP_CASES = {"counts_64": counts_64, "counts_128": counts_128, "counts_256": counts_256, "holes": holes,
                   "coarse_border": coarse_border, "leaving": leaving, "frame_600": frame_600}

_cache = {}


def case(name, *args):
    key = (name, args)
    if key not in _cache:
        fn = WORKGROUP_CASES.get(name) or globals()[name]
        b, sched = fn(*args)
        _cache[key] = [b, sched, None]
    return _cache[key]


def reference(oracle, name, *args):
    """(batch, schedule, the oracle's poses, its per-frame results) -- the oracle runs once per case and session"""
    c = case(name, *args)
    if c[2] is None:
        hi, lo, n_iter = c[1]
        T_o, res_o, _ = run_oracle(oracle, c[0], hi, lo, n_iter)
        c[2] = (T_o, res_o)
    return c[0], c[1], c[2][0], c[2][1]
