"""Which code an entry point returns for which bad argument, and that a valid call still launches: the seed entries of
depth_filter.hip, the pose entries of pose_optimizer.hip and the builders of pyramid.hip on the host-emulated library
(tests/emu_build.py).  A rejected call launches nothing, so a case takes milliseconds.  The expected codes are literals, read
off the entry points' checks: struct pointers and the batch size first (EINVAL), an empty batch next (OK), every other
EINVAL check, the workspace last (ERANGE); the pose entries test the range of n_stride (ERANGE) before the empty batch and
the arrays."""
import ctypes as C

import numpy as np
import pytest

from rpg_svo_amd import capi

OK, EINVAL, ERANGE = 0, -1, -2
W, H, N_LEVELS, S, B, N_STRIDE = 64, 48, 3, 4, 1, 8

SEED_ORDER = {
    "svo_hip_update_seeds": ("layout", "store", "cam", "frames", "S", "d_cur_frame", "ftr", "seeds", "opt", "d_status", "d_xyz_world",
                             "d_px_cur", "d_workspace", "workspace_bytes", "stream"),
    "svo_hip_update_seeds_resident": ("layout", "store", "cam", "frames", "cur_frame", "S", "d_slot_of", "ftr", "seeds", "opt", "d_status",
                                      "d_xyz_world", "d_px_cur", "d_state_out", "d_workspace", "workspace_bytes", "stream"),
    "svo_hip_update_seeds_resident_pose": ("layout", "store", "cam", "frames", "cur_frame", "T_cur_f_w", "S", "d_slot_of", "ftr", "seeds",
                                           "opt", "d_status", "d_xyz_world", "d_px_cur", "d_state_out", "d_workspace", "workspace_bytes",
                                           "stream"),
    "svo_hip_find_epipolar_match_direct": ("layout", "store", "cam", "frames", "S", "d_cur_frame", "ftr", "d_d_estimate", "d_d_min",
                                           "d_d_max", "opt", "d_ok", "d_depth", "d_px_cur", "d_search_level", "d_workspace",
                                           "workspace_bytes", "stream"),
}
UPDATE_ENTRIES = ("svo_hip_update_seeds", "svo_hip_update_seeds_resident", "svo_hip_update_seeds_resident_pose")
RESIDENT_ENTRIES = UPDATE_ENTRIES[1:]
SEED_ENTRIES = tuple(SEED_ORDER)
POSE_ORDER = ("cam", "B", "d_n", "n_stride", "d_f", "d_level", "d_pos", "d_has_point", "reproj_thresh", "n_iter", "d_T_f_w", "d_Cov",
              "d_stats", "d_ran", "stream")
POSE_ENTRIES = ("svo_hip_pose_optimize", "svo_hip_pose_optimize_deferred", "svo_hip_pose_optimize_ordered")
POSE_REQUIRED = ("d_n", "d_f", "d_level", "d_pos", "d_has_point", "d_T_f_w", "d_stats", "d_ran")
PYR_ORDER = {
    "svo_hip_pyramid_build": ("layout", "store", "first_slot", "n_slots", "halfsample_mode", "stream"),
    "svo_hip_pyramid_build_from_images": ("layout", "store", "first_slot", "n_slots", "images", "image_stride", "row_stride",
                                          "halfsample_mode", "stream"),
    "svo_hip_pyramid_build_tiled": ("layout", "store", "first_slot", "n_slots", "images", "image_stride", "row_stride", "halfsample_mode",
                                    "tile_width", "stream"),
    "svo_hip_pyramid_build_per_level": ("layout", "store", "first_slot", "n_slots", "halfsample_mode", "stream"),
    "svo_hip_pyramid_upload_build": ("layout", "store", "first_slot", "images", "row_stride", "halfsample_mode", "d_staging", "stream"),
}
PYR_ENTRIES = tuple(PYR_ORDER)
PYR_TAKES_IMAGES = ("svo_hip_pyramid_build_from_images", "svo_hip_pyramid_build_tiled", "svo_hip_pyramid_upload_build")
PYR_TAKES_SLOT_RANGE = PYR_ENTRIES[:4]

# the pointers an entry cannot do without (arguments, and fields of frames / ftr / seeds): nulling one gives EINVAL
_FRAMES_FTR = ("frames.d_slot", "frames.d_T_f_w", "ftr.d_frame", "ftr.d_level", "ftr.d_px", "ftr.d_f")
_SEED_FIELDS = ("seeds.d_a", "seeds.d_b", "seeds.d_mu", "seeds.d_z_range", "seeds.d_sigma2", "seeds.d_batch_id")
_STRUCTS = ("layout", "store", "cam", "frames", "ftr", "opt")
SEED_REQUIRED = {
    "svo_hip_update_seeds": _STRUCTS + ("seeds", "d_cur_frame", "d_status") + _FRAMES_FTR + _SEED_FIELDS,
    "svo_hip_update_seeds_resident": _STRUCTS + ("seeds", "d_slot_of", "d_status") + _FRAMES_FTR + _SEED_FIELDS,
    "svo_hip_update_seeds_resident_pose": _STRUCTS + ("seeds", "T_cur_f_w", "d_slot_of", "d_status") + _FRAMES_FTR + _SEED_FIELDS,
    "svo_hip_find_epipolar_match_direct": _STRUCTS + ("d_cur_frame", "d_d_estimate", "d_d_min", "d_d_max", "d_ok", "d_depth") + _FRAMES_FTR,
}
# what an empty batch may leave out: every per-seed array, the tables behind the structs, the workspace
SEED_ARRAYS = ("d_cur_frame", "d_slot_of", "d_status", "d_xyz_world", "d_px_cur", "d_state_out", "d_workspace", "d_d_estimate", "d_d_min",
               "d_d_max", "d_ok", "d_depth", "d_search_level", "ftr.d_type", "ftr.d_grad") + _FRAMES_FTR + _SEED_FIELDS


@pytest.fixture(scope="module")
def emu():
    from emu_build import build_emulated
    lib = build_emulated(())   # (a CDLL object of this module's own: the prototypes set here are seen by nobody else)
    for name in SEED_ENTRIES + POSE_ENTRIES + PYR_ENTRIES + ("svo_hip_match_workspace_bytes", "svo_hip_pyramid_load_level0",
                                                                "svo_hip_pyramid_download_level"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = capi.PROTOTYPES[name]
    return lib


def _arg(v):
    if isinstance(v, np.ndarray):
        return v.ctypes.data
    return C.byref(v) if isinstance(v, C.Structure) else v


def _call(emu, entry, order, args, changes=None):
    """entry(*args in `order`) with `changes` applied: {"name": value} replaces an argument, {"struct.field": value} a field
    of a copy of that struct"""
    a = dict(args)
    for k, v in (changes or {}).items():
        name, _, field = k.partition(".")
        if field:
            if a[name] is None:
                continue
            a[name] = type(a[name]).from_buffer_copy(a[name])
            setattr(a[name], field, v)
        else:
            a[name] = v
    return getattr(emu, entry)(*[_arg(a[n]) for n in order])


def _images(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, h, w), dtype=np.uint8)


@pytest.fixture(scope="module")
def store(emu):
    """one slot of a 64 x 48 pyramid of 3 levels"""
    layout = capi.pyr_layout(W, H, N_LEVELS)
    buf = np.zeros(capi.pyr_store_bytes(layout, 1), np.uint8)
    imgs = _images(1, H, W, 1)
    assert emu.svo_hip_pyramid_build_tiled(C.byref(layout), buf.ctypes.data, 0, 1, imgs.ctypes.data, H * W, W, capi.HALFSAMPLE_AUTO, 0, None) == OK
    return layout, buf


def _seed_args(emu, store):
    """S = 4 seeds of frame 0 seen again from frame 1 (both in slot 0, 0.1 apart), fresh arrays for every call"""
    layout, buf = store
    cam = capi.Camera(60.0, 60.0, 32.0, 24.0, W, H, 0, 0, (C.c_double * 5)())
    T = np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), (2, 1))
    T[1, 9] = 0.1
    slots = np.zeros(2, np.int32)
    px = np.array([[20.0 + 6.0 * i, 24.0] for i in range(S)])
    f = np.concatenate([(px - [32.0, 24.0]) / 60.0, np.ones((S, 1))], axis=1)
    f = np.ascontiguousarray(f / np.linalg.norm(f, axis=1, keepdims=True))
    k = dict(frame=np.zeros(S, np.int32), level=np.zeros(S, np.int32), type=np.zeros(S, np.uint8), px=px, f=f, grad=np.tile([1.0, 0.0], (S, 1)),
             a=np.full(S, 10, np.float32), b=np.full(S, 10, np.float32), mu=np.full(S, 0.5, np.float32), z_range=np.full(S, 1.0, np.float32),
             sigma2=np.full(S, 1.0 / 36, np.float32), batch_id=np.zeros(S, np.int32), T=T, slots=slots)
    ws = np.zeros(emu.svo_hip_match_workspace_bytes(S) + 256, np.uint8)
    ws = ws[(-ws.ctypes.data) % 256:][:emu.svo_hip_match_workspace_bytes(S)]
    return dict(
        layout=layout, store=buf, cam=cam, frames=capi.Frames(2, 0, slots.ctypes.data, T.ctypes.data), S=S, cur_frame=1,
        T_cur_f_w=T[1].copy(), d_cur_frame=np.ones(S, np.int32), d_slot_of=np.arange(S, dtype=np.int32),
        ftr=capi.Features(*[k[n].ctypes.data for n in ("frame", "level", "type", "px", "f", "grad")]),
        seeds=capi.Seeds(*[k[n].ctypes.data for n in ("a", "b", "mu", "z_range", "sigma2", "batch_id")]),
        opt=capi.DepthFilterOptions(3, 0, 200.0, 0, 10, 1000, 1, 1, N_LEVELS, 0.7),
        d_status=np.zeros(S, np.int32), d_xyz_world=np.zeros((S, 3)), d_px_cur=np.zeros((S, 2)), d_state_out=np.zeros((4, S), np.float32),
        d_d_estimate=np.full(S, 2.0), d_d_min=np.full(S, 1.5), d_d_max=np.full(S, 3.0), d_ok=np.zeros(S, np.int32), d_depth=np.zeros(S),
        d_search_level=np.zeros(S, np.int32), d_workspace=ws, workspace_bytes=ws.size, stream=None, _keep=k)


def _seed_call(emu, store, entry, changes=None):
    return _call(emu, entry, SEED_ORDER[entry], _seed_args(emu, store), changes)


@pytest.mark.parametrize("entry", SEED_ENTRIES)
def test_seed_entry_takes_a_valid_call(emu, store, entry):
    assert _seed_call(emu, store, entry) == OK


@pytest.mark.parametrize("entry", SEED_ENTRIES)
def test_seed_entry_required_pointers(emu, store, entry):
    for name in SEED_REQUIRED[entry]:
        assert _seed_call(emu, store, entry, {name: None}) == EINVAL, name
    assert _seed_call(emu, store, entry, {"d_workspace": None}) == ERANGE   # (the workspace answers with its own code)


@pytest.mark.parametrize("entry", SEED_ENTRIES)
def test_seed_entry_batch_size_and_empty_batch(emu, store, entry):
    nothing = {name: None for name in SEED_ARRAYS}
    assert _seed_call(emu, store, entry, {"S": -1}) == EINVAL
    assert _seed_call(emu, store, entry, {"S": 0, "workspace_bytes": 0, **nothing}) == OK
    if entry in UPDATE_ENTRIES:
        assert _seed_call(emu, store, entry, {"S": 0, "seeds": None}) == EINVAL   # struct pointers before the empty batch
    if entry == "svo_hip_update_seeds_resident_pose":
        assert _seed_call(emu, store, entry, {"S": 0, "T_cur_f_w": None}) == EINVAL   # (and this entry's pose before everything)


@pytest.mark.parametrize("entry", SEED_ENTRIES)
def test_seed_entry_options_and_feature_types(emu, store, entry):
    assert _seed_call(emu, store, entry, {"ftr.d_grad": None}) == EINVAL    # types without gradients
    assert _seed_call(emu, store, entry, {"ftr.d_grad": None, "ftr.d_type": None}) == OK   # (both optional together)
    for field, value in (("n_pyr_levels", 0), ("n_pyr_levels", N_LEVELS + 1), ("align_max_iter", -1), ("max_epi_search_steps", -1)):
        assert _seed_call(emu, store, entry, {"opt." + field: value}) == EINVAL, (field, value)


@pytest.mark.parametrize("entry", RESIDENT_ENTRIES)
def test_resident_seed_entry_current_frame(emu, store, entry):
    assert _seed_call(emu, store, entry, {"cur_frame": -1}) == EINVAL
    assert _seed_call(emu, store, entry, {"cur_frame": 2}) == EINVAL        # = frames.n_frames
    if entry.endswith("_pose"):
        assert _seed_call(emu, store, entry, {"T_cur_f_w": None}) == EINVAL


@pytest.mark.parametrize("entry", SEED_ENTRIES)
def test_seed_entry_workspace_comes_last(emu, store, entry):
    short = {"workspace_bytes": emu.svo_hip_match_workspace_bytes(S) - 1}
    verdict = "d_ok" if entry == "svo_hip_find_epipolar_match_direct" else "d_status"
    assert _seed_call(emu, store, entry, short) == ERANGE
    assert _seed_call(emu, store, entry, {**short, verdict: None}) == EINVAL   # null checks before the workspace check
    assert _seed_call(emu, store, entry, {**short, "opt.align_max_iter": -1}) == EINVAL
    assert _seed_call(emu, store, entry, {**short, "S": 0}) == OK             # (an empty batch needs none)


def _pose_args():
    rng = np.random.default_rng(2)
    pos = np.concatenate([rng.uniform(-0.5, 0.5, size=(N_STRIDE, 2)), rng.uniform(1.5, 2.5, size=(N_STRIDE, 1))], axis=1)
    f = pos + rng.normal(size=pos.shape) * 1e-3
    f = np.ascontiguousarray(f / np.linalg.norm(f, axis=1, keepdims=True))
    has = np.zeros(N_STRIDE, np.uint8)
    has[:4] = 1
    return dict(cam=capi.Camera(60.0, 60.0, 32.0, 24.0, W, H, 0, 0, (C.c_double * 5)()), B=B, d_n=np.full(B, 4, np.int32), n_stride=N_STRIDE,
                d_f=f, d_level=np.zeros(N_STRIDE, np.int32), d_pos=pos, d_has_point=has, reproj_thresh=2.0, n_iter=10,
                d_T_f_w=np.concatenate([np.eye(3).ravel(), np.zeros(3)]), d_Cov=np.zeros(36), d_stats=np.zeros(4), d_ran=np.zeros(B, np.int32),
                stream=None)


def _pose_call(emu, entry, changes=None):
    return _call(emu, entry, POSE_ORDER, _pose_args(), changes)


@pytest.mark.parametrize("entry", POSE_ENTRIES)
def test_pose_entry_return_codes(emu, entry):
    nothing = {name: None for name in POSE_REQUIRED + ("d_Cov",)}
    assert _pose_call(emu, entry) == OK
    assert _pose_call(emu, entry, {"d_Cov": None}) == OK                     # the covariance is optional
    assert _pose_call(emu, entry, {"cam": None}) == EINVAL
    assert _pose_call(emu, entry, {"cam.model": 7}) == EINVAL
    for name, value in (("B", -1), ("n_stride", 0), ("n_iter", -1)):
        assert _pose_call(emu, entry, {name: value}) == EINVAL, name
    # the range of n_stride: after the EINVAL checks of the scalars, before the empty batch and before the arrays
    assert _pose_call(emu, entry, {"n_stride": 1025}) == ERANGE
    assert _pose_call(emu, entry, {"n_stride": 1025, "B": 0}) == ERANGE
    assert _pose_call(emu, entry, {"n_stride": 1025, **nothing}) == ERANGE
    assert _pose_call(emu, entry, {"n_stride": 1025, "n_iter": -1}) == EINVAL
    assert _pose_call(emu, entry, {"B": 0, **nothing}) == OK
    for name in POSE_REQUIRED:
        assert _pose_call(emu, entry, {name: None}) == EINVAL, name


def _pyr_args(store):
    layout, _ = store
    buf = np.zeros(capi.pyr_store_bytes(layout, 1), np.uint8)
    return dict(layout=layout, store=buf, first_slot=0, n_slots=1, images=_images(1, H, W, 3), image_stride=H * W, row_stride=W,
                halfsample_mode=capi.HALFSAMPLE_AUTO, tile_width=0, d_staging=None, stream=None)


def _pyr_call(emu, store, entry, changes=None):
    return _call(emu, entry, PYR_ORDER[entry], _pyr_args(store), changes)


@pytest.mark.parametrize("entry", PYR_ENTRIES)
def test_pyramid_entry_return_codes(emu, store, entry):
    assert _pyr_call(emu, store, entry) == OK
    assert _pyr_call(emu, store, entry, {"halfsample_mode": -1}) == EINVAL
    assert _pyr_call(emu, store, entry, {"halfsample_mode": 3}) == EINVAL
    assert _pyr_call(emu, store, entry, {"first_slot": -1}) == EINVAL        # (the upload entry's one slot too)
    if entry in PYR_TAKES_IMAGES:
        assert _pyr_call(emu, store, entry, {"row_stride": W - 1}) == EINVAL
    if entry in PYR_TAKES_SLOT_RANGE:
        assert _pyr_call(emu, store, entry, {"n_slots": -1}) == EINVAL
        assert _pyr_call(emu, store, entry, {"n_slots": 0}) == OK
    if entry == "svo_hip_pyramid_build_tiled":
        assert _pyr_call(emu, store, entry, {"tile_width": 300}) == EINVAL
        assert _pyr_call(emu, store, entry, {"images": None, "row_stride": 0}) == OK   # (level 0 already in the store)


@pytest.mark.parametrize("mode", [capi.HALFSAMPLE_SCALAR, capi.HALFSAMPLE_SSE2, capi.HALFSAMPLE_AUTO])
def test_levels_beyond_the_fused_ones_are_the_per_level_builders(emu, mode):
    """6 levels of a 320 x 240 image: the fused kernel builds 5, the sixth comes from the per-level loop behind it -- the bytes
    svo_hip_pyramid_build_per_level writes there."""
    w, h, n_levels, n = 320, 240, 6, 2
    layout = capi.pyr_layout(w, h, n_levels)
    imgs = _images(n, h, w, 4 + mode)
    got = []
    for fused in (True, False):
        buf = np.zeros(capi.pyr_store_bytes(layout, n), np.uint8)
        if fused:
            rc = emu.svo_hip_pyramid_build_tiled(C.byref(layout), buf.ctypes.data, 0, n, imgs.ctypes.data, h * w, w, mode, 0, None)
        else:
            assert emu.svo_hip_pyramid_load_level0(C.byref(layout), buf.ctypes.data, 0, n, imgs.ctypes.data, h * w, w, None) == OK
            rc = emu.svo_hip_pyramid_build_per_level(C.byref(layout), buf.ctypes.data, 0, n, mode, None)
        assert rc == OK
        levels = []
        for slot in range(n):
            for lvl in (4, 5):
                out = np.zeros((layout.h[lvl], layout.w[lvl]), np.uint8)
                assert emu.svo_hip_pyramid_download_level(C.byref(layout), buf.ctypes.data, slot, lvl, out.ctypes.data, None) == OK
                levels.append(out)
        got.append(levels)
    assert got[0][1].shape == (7, 10) and got[0][1].std() > 1.0             # (a picture, not a blank)
    for a, b in zip(*got):
        assert np.array_equal(a, b)
