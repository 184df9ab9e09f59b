"""The literal drop-in: the reference's svo::FrameHandlerMono (its own translation units for
the control plane, compiled against oracle/shim) run twice on one synthetic sequence --

  ref: every translation unit is the reference's                      (CPU reference path)
  hip: sparse_img_align / reprojector / pose_optimizer / depth_filter / feature_detection are the bodies of
       rpg_svo_amd/host/dropin/*.cpp, which call libsvo_hip.so        (the product)

and the two trajectories compared frame by frame (BASELINE.json metric: "ATE vs CPU ref",
SE(3) log-map norm).  The libraries are built by tests/dropin/Makefile where the reference
checkout exists (this container) and travel prebuilt to the GPU box.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "dropin"))
import pypipeline as pp  # noqa: E402

from rpg_svo_amd import se3, synth  # noqa: E402

# stated tolerances (hip vs CPU reference, same images)
SE3_LOGNORM_TOL = 1e-4   # per frame
# With N(0, 2) image noise the last accepted Gauss-Newton step of sparse alignment is ~1e-4 itself;
# tree- vs sequentially-summed chi2 can flip the reference's `new_chi2 > chi2` stop test, which leaves the
# two runs ONE step apart for a frame (the later stages pull the pose back: median stays ~1e-8).
SE3_LOGNORM_TOL_NOISY = 3e-4
# Horn-aligned RMSE over the sequence, scene depth 2 m.  The per-frame deviation is 1e-9..1e-8 except on the
# frames where the stop test of sparse alignment flips (single frames at 1e-6..6e-5, scripts/dropin_frame_debug.py);
# those spikes are the whole of the RMSE, so its bound follows the per-frame bound (1.2e-5 measured).
ATE_TOL_M = 5e-5


def _sequence(n_frames, seed=5, cam=None):
    default_cam = cam is None
    cam = cam or synth.Camera(752, 480, 315.5, 315.5, 376.0, 240.0)  # svo/test/test_pipeline.cpp:46-47 intrinsics
    # child processes of one test share the parent's rendering (SVO_TEST_SEQ_FILE: the default sequence, at least this long;
    # a shorter sequence is a prefix of a longer one: the trajectory is a seeded walk, a frame depends on its pose only)
    f = os.environ.get("SVO_TEST_SEQ_FILE")
    if f and default_cam and seed == 5 and os.path.exists(f):
        d = np.load(f)
        if d["T"].shape[0] >= n_frames:
            return cam, np.ascontiguousarray(d["imgs"][:n_frames]), np.ascontiguousarray(d["T"][:n_frames])
    tex = synth.make_texture(seed=12345)
    T = synth.make_trajectory(n_frames, seed=seed, max_step=0.02, max_rot_deg=0.3)
    return cam, synth.render(tex, T, cam).numpy(), T


def _horn_ate(P, Q):
    Pc, Qc = P - P.mean(0), Q - Q.mean(0)
    U, _, Vt = np.linalg.svd((Pc.T @ Qc).T)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1
    R = U @ S @ Vt
    t = Q.mean(0) - R @ P.mean(0)
    return float(np.sqrt((((R @ P.T).T + t - Q) ** 2).sum(1).mean()))


@pytest.fixture(scope="module")
def pipeline_libs():
    pp.build("all")  # no-op without /root/reference
    if not (pp.available("ref") and pp.available("hip")):
        pytest.skip("tests/dropin/_build/*.so absent and no reference checkout to build them from")
    return True


def test_reference_pipeline_tracks_on_cpu(pipeline_libs):
    """Pins the harness: the reference's own pipeline follows the synthetic sequence, selects
    keyframes, converges seeds -- i.e. the comparison below exercises the whole path."""
    cam, imgs, T = _sequence(60)
    res = pp.run_sequence("ref", cam, imgs, T)
    assert res[0]["n_first_features"] > 200
    assert all(r["stage"] == pp.STAGE_DEFAULT_FRAME for r in res)
    est = np.stack([r["T_f_w"] for r in res])
    assert se3.log_norm(est, T).max() < 5e-3
    assert sum(r["is_keyframe"] for r in res) >= 3
    assert max(r["n_candidates"] for r in res) > 50      # depth-filter seeds converged into candidates
    assert all(r["repr_n_new_references"] >= 100 for r in res[1:])


def test_dropin_library_links_every_symbol(pipeline_libs):
    """dlopen with RTLD_NOW: every reference symbol the control plane needs from the four
    replaced translation units is provided by the drop-in bodies (no compute: no GPU here)."""
    import ctypes
    lib = ctypes.CDLL(pp.lib_path("hip"), mode=os.RTLD_NOW)
    for name in ("pipe_create", "pipe_set_first_frame", "pipe_add_image", "pipe_destroy"):
        assert hasattr(lib, name)


# ---- the drop-ins' HOST code on a mock device (CPU suite) ------------------------------------------------------------
# tests/dropin/_build/libsvo_pipeline_hipmock.so links the same objects as the hip flavour -- the reference's control
# plane + rpg_svo_amd/host/dropin/*.cpp + svo_hip_device.cpp -- against tests/host/mock_svo_hip.cpp and
# tests/dropin/mock_compute_oracle.cpp (the C ABI served by host memory and the CPU oracle) instead of libsvo_hip.so.
# Everything the host layer decides -- marshalling, trial order, the predicted pose refinement and its verification, the
# deferred mapper's replay, slot pinning and eviction -- is therefore exercised here, where there is no GPU; the
# arithmetic is the oracle's, so the trajectory must follow the reference's own to rounding (poses cross the boundary as
# rotation matrices, sparse alignment gets f * depth instead of f and depth: 1e-15 per frame, 1e-8 after 80 frames).
MOCK_TOL = 1e-7


@pytest.fixture(scope="module")
def mock_lib(pipeline_libs):
    if not pp.available("hipmock"):
        pytest.skip("tests/dropin/_build/libsvo_pipeline_hipmock.so absent and no reference checkout to build it from")
    return True


def _same_decisions(a, b, keys=("is_keyframe", "n_obs", "repr_n_mps", "repr_n_new_references", "n_kfs", "stage", "img_align_n_tracked")):
    for k in keys:
        assert [r[k] for r in a] == [r[k] for r in b], k


def test_dropin_host_logic_on_the_mock_device(mock_lib):
    cam, imgs, T = _sequence(80)
    ref = pp.run_sequence("ref", cam, imgs, T)
    st = {}
    mock = pp.run_sequence("hipmock", cam, imgs, T, stats_out=st)
    d = se3.log_norm(np.stack([r["T_f_w"] for r in mock]), np.stack([r["T_f_w"] for r in ref]))
    assert d.max() <= MOCK_TOL, d.max()
    _same_decisions(ref, mock, ("is_keyframe", "n_obs", "repr_n_mps", "repr_n_new_references", "n_kfs", "stage",
                                "img_align_n_tracked", "n_seeds", "n_candidates", "sfba_n_edges_final"))
    assert sum(r["is_keyframe"] for r in mock) >= 3 and max(r["n_candidates"] for r in mock) > 50
    # every frame's pose refinement was the one the reprojector predicted and enqueued
    assert st["predicted_pose_misses"] == 0 and st["predicted_pose_hits"] == len(imgs) - 1
    assert st["uploads"] == len(imgs) and st["evictions"] == len(imgs) - 64  # 64 slots: old frames leave, none comes back


def test_dropin_sparse_align_says_no_to_levenberg_marquardt(mock_lib):
    """vk::NLLSSolver offers two methods (sparse_img_align.h:43-49); the reference pipeline constructs GaussNewton only
    (frame_handler_mono.cpp:136-137) and the kernel runs that loop.  The drop-in's constructor must refuse the other one
    instead of silently running Gauss-Newton (as the Python mirror does); the all-CPU reference accepts both."""
    import ctypes
    for flavour, expect in (("ref", 0), ("hipmock", 1)):
        lib = ctypes.CDLL(pp.lib_path(flavour))
        lib.pipe_sparse_align_rejects_levenberg_marquardt.restype = ctypes.c_int
        assert lib.pipe_sparse_align_rejects_levenberg_marquardt() == expect, flavour


def test_full_dropin_builds_no_host_pyramid(mock_lib):
    """rpg_svo_amd/host/dropin/frame.cpp: in the full drop-in every reader of the host pyramid's upper levels is a drop-in,
    so frame_utils::createImgPyramid keeps level 0 and leaves the rest empty (the reference builds them all: three to five
    halfSample passes per frame nobody reads) -- same decisions, same trajectory as with the levels built
    (SVO_HIP_HOST_PYRAMID=1, read once per process: a child)."""
    import json
    import subprocess
    cam, imgs, T = _sequence(40)
    st = {}
    res = pp.run_sequence("hipmock", cam, imgs, T, stats_out=st)
    n_levels, filled = st["host_pyramid"]
    assert n_levels >= 5 and filled == 1, st["host_pyramid"]
    st_ref = {}
    pp.run_sequence("ref", cam, imgs[:3], T[:3], stats_out=st_ref)
    assert st_ref["host_pyramid"] == (n_levels, n_levels)           # the reference's own frame.cpp
    code = ("import sys, json, numpy as np\n"
            f"sys.path.insert(0, {HERE!r}); sys.path.insert(0, {os.path.join(HERE, 'dropin')!r})\n"
            "import pypipeline as pp\n"
            "from test_dropin_pipeline import _sequence\n"
            "cam, imgs, T = _sequence(40)\n"
            "st = {}\n"
            "res = pp.run_sequence('hipmock', cam, imgs, T, stats_out=st)\n"
            "print(json.dumps(dict(pyr=st['host_pyramid'], T=[list(map(float, r['T_f_w'])) for r in res], kf=[int(r['is_keyframe']) for r in res])))\n")
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SVO_HIP_HOST_PYRAMID="1"), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    other = json.loads(p.stdout.strip().splitlines()[-1])
    assert tuple(other["pyr"]) == (n_levels, n_levels)
    assert np.array_equal(np.array(other["T"]), np.stack([r["T_f_w"] for r in res]))
    assert other["kf"] == [int(r["is_keyframe"]) for r in res]


def test_mock_device_deferred_mapper_and_small_pool(mock_lib):
    """Deferred mapping (results of DepthFilter::updateSeeds joined at the next reprojectMap / updateSeeds / detect) and
    a pyramid pool so small that live frames are evicted and uploaded again: the trajectory must not notice either."""
    cam, imgs, T = _sequence(80)
    base = pp.run_sequence("hipmock", cam, imgs, T)
    Tb = np.stack([r["T_f_w"] for r in base])
    deferred = pp.run_sequence("hipmock", cam, imgs, T, defer_mapper=1)
    assert np.array_equal(np.stack([r["T_f_w"] for r in deferred]), Tb)
    _same_decisions(base, deferred)
    assert sum(r["n_candidates"] for r in deferred) > 0
    st = {}
    small = pp.run_sequence("hipmock", cam, imgs, T, stats_out=st, pool_slots=7, defer_mapper=1)
    assert np.array_equal(np.stack([r["T_f_w"] for r in small]), Tb)
    assert st["evictions"] > 50 and st["uploads"] >= len(imgs)
    # a sequence after a deferred one in the same process: nothing pending leaks into the next handler
    again = pp.run_sequence("hipmock", cam, imgs[:30], T[:30])
    assert np.array_equal(np.stack([r["T_f_w"] for r in again]), Tb[:30])


def test_mock_device_tracking_loss_and_relocalization(mock_lib):
    """The scenario of test_tracking_loss_and_relocalization on the mock device: a prediction enqueued for a frame whose
    pose refinement never comes (RESULT_FAILURE) must be dropped by the lane's next call, relocalization runs the
    sparse alignment outside processFrame, and the deferred mapper meets FrameHandlerMono's reset paths."""
    cam, imgs, T = _sequence(52, seed=9)
    k0 = 36
    T2 = se3.mul(T, np.broadcast_to(se3.inv(T[k0][None])[0], T.shape).copy())
    imgs = imgs.copy()
    imgs[30:33] = 0
    r0 = pp.range_map(cam, T[0])
    ref = pp.run_sequence("ref", cam, imgs, T2, range0=r0)
    for defer in (0, 1):
        st = {}
        mock = pp.run_sequence("hipmock", cam, imgs, T2, range0=r0, stats_out=st, defer_mapper=defer)
        assert [r["stage"] for r in mock] == [r["stage"] for r in ref]
        assert [r["stage"] for r in ref][30:34] == [pp.STAGE_RELOCALIZING] * 3 + [pp.STAGE_DEFAULT_FRAME]
        _same_decisions(ref, mock, ("is_keyframe", "n_obs", "repr_n_new_references", "img_align_n_tracked"))
        d = se3.log_norm(np.stack([r["T_f_w"] for r in mock]), np.stack([r["T_f_w"] for r in ref]))
        assert d.max() <= MOCK_TOL, (defer, d.max())
        assert st["predicted_pose_hits"] > 40


@pytest.mark.parametrize("kind", ["atan", "radtan"])
def test_mock_device_with_the_reference_launch_file_cameras(mock_lib, kind):
    """Camera recovery through the abstract interface, device cam2world for the predicted observations, distorted models."""
    from helpers import camera_models
    cam = camera_models()[kind]
    cam_, imgs, T = _sequence(40, cam=cam)
    ref = pp.run_sequence("ref", cam, imgs, T)
    st = {}
    mock = pp.run_sequence("hipmock", cam, imgs, T, stats_out=st)
    d = se3.log_norm(np.stack([r["T_f_w"] for r in mock]), np.stack([r["T_f_w"] for r in ref]))
    # (the camera's parameters are recovered by probing world2cam through the abstract interface: 1e-12 relative, and the
    # radial-tangential cam2world rounds to float)
    assert d.max() <= 1e-5, d.max()
    _same_decisions(ref, mock)
    assert st["predicted_pose_misses"] == 0


def test_mock_device_with_the_mapping_thread(mock_lib):
    """DepthFilter's own thread running: tracking lane and mapping lane of two host threads, deferral off by itself
    (thread_ != NULL).  Timing dependent like the reference: checked against ground truth."""
    cam, imgs, T = _sequence(80)
    for _ in range(2):
        mock = pp.run_sequence("hipmock", cam, imgs, T, mapper_thread=1, defer_mapper=1)
        est = np.stack([r["T_f_w"] for r in mock])
        assert all(r["stage"] == pp.STAGE_DEFAULT_FRAME for r in mock)
        assert se3.log_norm(est, T).max() < 5e-3
        assert sum(r["is_keyframe"] for r in mock) >= 3


def test_mock_device_arena_modes_and_no_prediction(mock_lib, tmp_path):
    """SVO_HIP_ARENA = hybrid / mirrored / mapped, SVO_HIP_SPECULATE = 0, a first match batch too small to reach the
    visiting loop's stop (all fixed when a lane / the process starts: one process each): the host code paths differ --
    where blocks live, which copies are issued, polling a signal or waiting for a stream, prediction on the same or on a
    second stream or none -- the results do not."""
    import subprocess
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {HERE!r}); sys.path.insert(0, {os.path.join(HERE, 'dropin')!r})\n"
        "import pypipeline as pp\n"
        "import test_dropin_pipeline as t\n"
        "cam, imgs, T = t._sequence(50)\n"
        "st = {}\n"
        "r = pp.run_sequence('hipmock', cam, imgs, T, stats_out=st)\n"
        "np.save(sys.argv[1], np.stack([x['T_f_w'] for x in r]))\n"
        "print(st['predicted_pose_hits'], st['predicted_pose_misses'])\n")
    from concurrent.futures import ThreadPoolExecutor
    _, imgs_, T_ = _sequence(50)                        # rendered once, here; the children load it and start together
    seq_file = str(tmp_path / "sequence.npz")
    np.savez(seq_file, imgs=imgs_, T=T_)
    out, hits = {}, {}

    def child(name, env):
        path = str(tmp_path / f"traj_{name}.npy")
        p = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, SVO_TEST_SEQ_FILE=seq_file, **env), capture_output=True,
                           text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        return np.load(path), [int(x) for x in p.stdout.split()[-2:]]

    modes = (("hybrid", {}), ("mirrored", {"SVO_HIP_ARENA": "mirrored"}), ("mapped", {"SVO_HIP_ARENA": "mapped"}),
             ("no_prediction", {"SVO_HIP_SPECULATE": "0"}), ("second_batch", {"SVO_HIP_FIRST_BATCH_CELLS": "40"}))
    with ThreadPoolExecutor(max_workers=len(modes)) as ex:
        for (name, _), res in zip(modes, ex.map(lambda m: child(*m), modes)):
            out[name], hits[name] = res
    for name in ("mirrored", "mapped", "no_prediction", "second_batch"):
        assert np.array_equal(out[name], out["hybrid"]), name
    assert hits["hybrid"] == [49, 0] and hits["mirrored"] == [49, 0] and hits["mapped"] == [49, 0] and hits["no_prediction"] == [0, 0]
    # a first batch of 40 cells never reaches the stop at 121 matches: the rest of the cells goes in a second batch and the
    # prediction made on the first one is dropped, every frame
    assert hits["second_batch"] == [0, 0]


def test_mock_device_two_cameras_of_different_geometry(mock_lib):
    """Two FrameHandlerMono instances (752x480 and 640x480) fed alternately in one process: one device context per image
    geometry, each with its own store layout, lanes and predictions; deferred mapping on for both."""
    cam_a, imgs_a, T_a = _sequence(40)
    cam_b = synth.Camera(640, 480, 400.0, 400.0, 320.0, 240.0)
    T_b = synth.make_trajectory(40, seed=9, max_step=0.02, max_rot_deg=0.3)
    imgs_b = synth.render(synth.make_texture(seed=12345), T_b, cam_b).numpy()
    ref_a = pp.run_sequence("ref", cam_a, imgs_a, T_a)
    ref_b = pp.run_sequence("ref", cam_b, imgs_b, T_b)
    pa, pb = pp.Pipeline("hipmock", cam_a, defer_mapper=1), pp.Pipeline("hipmock", cam_b, defer_mapper=1)
    try:
        pa.set_first_frame(imgs_a[0], 0.0, T_a[0], pp.range_map(cam_a, T_a[0]))
        pb.set_first_frame(imgs_b[0], 0.0, T_b[0], pp.range_map(cam_b, T_b[0]))
        for i in range(1, 40):
            ra = pa.add_image(imgs_a[i], float(i))
            rb = pb.add_image(imgs_b[i], float(i))
            assert se3.log_norm(ra["T_f_w"][None], ref_a[i]["T_f_w"][None])[0] <= MOCK_TOL
            assert se3.log_norm(rb["T_f_w"][None], ref_b[i]["T_f_w"][None])[0] <= MOCK_TOL
            assert ra["is_keyframe"] == ref_a[i]["is_keyframe"] and rb["is_keyframe"] == ref_b[i]["is_keyframe"]
            assert ra["n_obs"] == ref_a[i]["n_obs"] and rb["n_obs"] == ref_b[i]["n_obs"]
    finally:
        pa.close()
        pb.close()


def test_mock_device_pool_too_small_is_an_error(mock_lib):
    """Two pyramid slots for a pipeline that needs the current frame and its reference keyframes resident at once: the
    host layer refuses (svo_hip::Error names the remedy) instead of evicting a frame a running call uses."""
    cam, imgs, T = _sequence(12)
    with pytest.raises(RuntimeError, match="larger pool"):
        pp.run_sequence("hipmock", cam, imgs, T, pool_slots=2)
    ok = pp.run_sequence("hipmock", cam, imgs, T)  # the context recovers with the next pipeline's own pool
    assert all(r["stage"] == pp.STAGE_DEFAULT_FRAME for r in ok)


def test_mock_device_standalone_seams(mock_lib):
    """Flavour "hipm" on the mock device: the reference's own Reprojector / DepthFilter / FastDetector calling the drop-in
    Matcher::findMatchDirect / findEpipolarMatchDirect (one trial per call) and feature_alignment::align1D / align2D --
    their marshalling (one Feature, one frame pair, scratch slots for stand-alone images) against the all-reference run."""
    if not pp.available("hipmmock"):
        pytest.skip("tests/dropin/_build/libsvo_pipeline_hipmmock.so not built")
    cam, imgs, T = _sequence(45, seed=5)
    ref = pp.run_sequence("ref", cam, imgs, T)
    mock = pp.run_sequence("hipmmock", cam, imgs, T)
    d = se3.log_norm(np.stack([r["T_f_w"] for r in mock]), np.stack([r["T_f_w"] for r in ref]))
    assert d.max() <= MOCK_TOL, d.max()
    _same_decisions(ref, mock, ("is_keyframe", "n_obs", "repr_n_mps", "repr_n_new_references", "n_kfs", "stage",
                                "img_align_n_tracked", "n_seeds", "n_candidates"))


def test_mock_device_detect_creates_no_feature_for_an_empty_cell(mock_lib):
    """The drop-in FastDetector::detect (flavour "hipmock": the one flavour on the mock device that links it; "hipm" keeps the
    reference's detector) at Config::triangMinCornerScore() = 20.1, whose float lies above the double: the empty cells of
    tests/fast_cases.py's case E hold a score that passes "score > threshold", and still exactly the cells with level >= 0
    become features -- none at (-1, -1), none with a negative level."""
    import fast_cases as fc
    for thresh in (20.1, 20.0):
        c = fc.case_empty(thresh, occupied=False)
        xy, lvl, _ = (a[0] for a in c.expected())
        has = lvl >= 0
        assert has.sum() == 4 and c.oracle_n_features(0) == (6 if thresh == 20.1 else 4)
        cam = synth.Camera(c.w, c.h, 80.0, 80.0, c.w / 2.0, c.h / 2.0)
        p = pp.Pipeline("hipmock", cam, n_pyr_levels=c.n_levels, grid_size=c.cell, triang_min_corner_score=thresh)
        try:
            T0 = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 2.0])
            n, _ = p.set_first_frame(c.images[0], 0.0, T0, np.full((c.h, c.w), 2.0, np.float32))
            px, level, _ = p.last_features()
        finally:
            p.close()
        assert n == len(px) == 4
        assert (level >= 0).all() and (px >= 0).all()
        assert np.array_equal(px, xy[has].astype(np.float64)) and np.array_equal(level, lvl[has])


MIRROR_CODE = (
    "import sys, json, numpy as np\n"
    "sys.path.insert(0, {here!r}); sys.path.insert(0, {dropin!r})\n"
    "import pypipeline as pp\n"
    "import test_dropin_pipeline as t\n"
    "cam, imgs, T = t._sequence({n})\n"
    "st = {{}}\n"
    "r = pp.run_sequence({flavour!r}, cam, imgs, T, stats_out=st, **{cfg!r})\n"
    "np.save(sys.argv[1], np.stack([x['T_f_w'] for x in r]))\n"
    "print(json.dumps(dict(st['map_mirror'], hits=st['predicted_pose_hits'], kfs=int(sum(x['is_keyframe'] for x in r)),\n"
    "                      chain_hits=st['frame_chain_hits'], chain_misses=st['frame_chain_misses'],\n"
    "                      early_taken=st['early_mapper_taken'], early_dropped=st['early_mapper_dropped'], early_two_phase=st['early_mapper_two_phase'],\n"
    "                      seed_store=st.get('seed_store'), seeds=[x['n_seeds'] for x in r],\n"
    "                      counts=[[x['repr_n_mps'], x['repr_n_new_references'], x['n_kf_points_in_frame'], x['n_candidates']] for x in r])))\n")


def _run_mirror(flavour, n, env, tmp_path, tag, **cfg):
    import json
    import subprocess
    path = str(tmp_path / f"traj_{tag}.npy")
    code = MIRROR_CODE.format(here=HERE, dropin=os.path.join(HERE, "dropin"), n=n, flavour=flavour, cfg=cfg)
    p = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    return np.load(path), json.loads(p.stdout.strip().splitlines()[-1])


def test_mock_device_map_mirror_is_the_list_walk(mock_lib, tmp_path):
    """Row N2, host side (rpg_svo_amd/host/dropin/map_mirror.h): Reprojector::reprojectMap on the device-resident mirror of
    the map against the list-walking path (SVO_HIP_MAP_MIRROR=off) on a sequence with keyframe insertions AND removals
    (max_n_kfs = 4): bit-identical trajectories, the same trials / matches / projected keyframe points / candidates in
    every frame.  `verify` re-walks the reference's pointer graph on every call and throws on the first record the
    incremental protocol missed (positions moved by Point::optimize, types changed and points deleted by the cell loop,
    candidates appended by the depth filter's callback, candidates deleted for failing to reproject).  The mode is
    read once per process."""
    from concurrent.futures import ThreadPoolExecutor
    n = 220
    V = {"SVO_HIP_MAP_MIRROR": "verify"}
    runs = {  # independent child processes: started together
        "off": ("hipmock", n, {"SVO_HIP_MAP_MIRROR": "off"}, dict(max_n_kfs=4)),
        "verify": ("hipmock", n, V, dict(max_n_kfs=4)),
        "sb": ("hipmock", 60, dict(V, SVO_HIP_FIRST_BATCH_CELLS="40"), {}),
        "off60": ("hipmock", 60, {"SVO_HIP_MAP_MIRROR": "off"}, {}),
        "thr": ("hipmock", 100, V, dict(mapper_thread=1)),
        "cap": ("hipmock", 60, dict(V, SVO_HIP_MIRROR_TRIALS="64"), {}),
        "small": ("hipmock", 130, V, dict(pool_slots=7)),
        "off130": ("hipmock", 130, {"SVO_HIP_MAP_MIRROR": "off"}, dict(pool_slots=7)),
    }
    cam_, imgs_, T_ = _sequence(n)                      # rendered once, here; the children load it
    seq_file = str(tmp_path / "sequence.npz")
    np.savez(seq_file, imgs=imgs_, T=T_)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        fut = {tag: ex.submit(_run_mirror, fl, k, dict(env, SVO_TEST_SEQ_FILE=seq_file), tmp_path, tag, **cfg)
               for tag, (fl, k, env, cfg) in runs.items()}
        res = {tag: f.result() for tag, f in fut.items()}
    (off, s_off), (ver, s_ver) = res["off"], res["verify"]
    assert np.array_equal(ver, off)
    assert s_ver["counts"] == s_off["counts"]
    assert s_off["calls"] == 0
    assert s_ver["calls"] == n - 1 and s_ver["fallbacks"] == 0 and s_ver["hits"] == n - 1
    assert s_ver["kfs"] >= 6                                       # more keyframes than the map holds: removals happened
    assert s_ver["kfs"] - 1 <= s_ver["rebuilds"] <= s_ver["kfs"] + 1   # one walk of the graph per keyframe, none in between
    # between keyframes a frame sends a handful of records, not the map
    per_frame = (s_ver["point_records_sent"] - s_ver["rebuilds"] * 600) / n
    assert per_frame < 60, s_ver
    # the second batch (the first one too small to reach the visiting loop's stop) continues on the mirror
    (sb, s_sb), (ref60, _) = res["sb"], res["off60"]
    assert np.array_equal(sb, ref60) and s_sb["second_batches"] >= 50 and s_sb["fallbacks"] == 0
    # the depth filter on its own thread appends candidates while the tracker runs (timing dependent: no frame-by-frame
    # comparison, but verify must hold -- it tolerates only candidates that arrived after the call's tail read)
    _, s_thr = res["thr"]
    assert s_thr["calls"] == 99 and s_thr["fallbacks"] == 0
    # a batch with more trials than the call has room for (capacity forced down to 64): the kernel reports it, what was
    # enqueued behind it is dropped and the frame takes the list-walking path -- every frame here
    cap, s_cap = res["cap"]
    assert np.array_equal(cap, ref60) and s_cap["fallbacks"] >= 55 and s_cap["hits"] == 59
    # a pool that cannot hold every keyframe at once: the frame takes the list-walking path (which pins only the
    # keyframes that serve as reference), same result
    (small, s_small), (ref130, _) = res["small"], res["off130"]
    assert np.array_equal(small, ref130) and 0 < s_small["fallbacks"] < 129   # (mirrored while the keyframes still fit)


@pytest.mark.gpu
def test_dropin_trajectory_matches_cpu_reference(pipeline_libs, gpu_device):
    cam, imgs, T = _sequence(120)
    ref = pp.run_sequence("ref", cam, imgs, T)
    st = {}
    hip = pp.run_sequence("hip", cam, imgs, T, stats_out=st)
    Tr = np.stack([r["T_f_w"] for r in ref])
    Th = np.stack([r["T_f_w"] for r in hip])
    d = se3.log_norm(Th, Tr)
    ate = _horn_ate(se3.inv(Th)[:, 9:], se3.inv(Tr)[:, 9:])
    print(f"drop-in vs CPU reference over {len(imgs)} frames: SE3 log-norm max {d.max():.3e} median {np.median(d):.3e}; "
          f"ATE {ate:.3e} m; keyframes {sum(r['is_keyframe'] for r in ref)}; pose refinements taken from the reprojector's "
          f"prediction {st['predicted_pose_hits']}, not taken {st['predicted_pose_misses']}")
    # every frame's pose refinement was enqueued behind its match kernels, with the device picking the host's features
    assert st["predicted_pose_misses"] == 0 and st["predicted_pose_hits"] == len(imgs) - 1
    assert d.max() <= SE3_LOGNORM_TOL
    assert ate <= ATE_TOL_M
    # same decisions: keyframes at the same frames, same match / tracking counts
    assert [r["is_keyframe"] for r in ref] == [r["is_keyframe"] for r in hip]
    for k in ("n_obs", "repr_n_mps", "repr_n_new_references", "sfba_n_edges_final", "img_align_n_tracked"):
        same = np.mean([a[k] == b[k] for a, b in zip(ref, hip)])
        assert same >= 0.97, (k, same)
    # seeds converge at most a frame apart
    assert np.mean([abs(a["n_seeds"] - b["n_seeds"]) <= 2 for a, b in zip(ref, hip)]) >= 0.97
    assert all(r["stage"] == pp.STAGE_DEFAULT_FRAME for r in hip)


@pytest.mark.gpu
def test_tracking_loss_and_relocalization(pipeline_libs, gpu_device):
    """FrameHandlerMono::relocalizeFrame (frame_handler_mono.cpp:237-265), the second production caller of
    SparseImgAlign: three blank frames lose tracking (RESULT_FAILURE -> STAGE_RELOCALIZING), every frame handed in
    while relocalizing is aligned against the closest keyframe starting from the IDENTITY world pose (a fresh
    Frame's T_f_w_), and processFrame runs again when more than 30 patches were tracked.  The world is chosen so
    that the camera is near the identity when the images come back, i.e. relocalization succeeds.  Both flavours
    must take the same stage transitions frame by frame."""
    cam, imgs, T = _sequence(52, seed=9)
    k0 = 36
    T2 = se3.mul(T, np.broadcast_to(se3.inv(T[k0][None])[0], T.shape).copy())  # frame k0 sits at the identity
    imgs = imgs.copy()
    imgs[30:33] = 0
    r0 = pp.range_map(cam, T[0])
    ref = pp.run_sequence("ref", cam, imgs, T2, range0=r0)
    hip = pp.run_sequence("hip", cam, imgs, T2, range0=r0)
    st_ref, st_hip = [r["stage"] for r in ref], [r["stage"] for r in hip]
    assert st_ref[30:33] == [pp.STAGE_RELOCALIZING] * 3, st_ref      # the scenario does what it is meant to
    assert st_ref[33] == pp.STAGE_DEFAULT_FRAME, st_ref              # ... and relocalizes with the first good image
    assert st_hip == st_ref
    assert [r["is_keyframe"] for r in ref] == [r["is_keyframe"] for r in hip]
    for k in ("n_obs", "repr_n_new_references", "img_align_n_tracked"):
        assert np.mean([a[k] == b[k] for a, b in zip(ref, hip)]) >= 0.95, k
    # SparseImgAlign inside relocalizeFrame did run in the hip flavour (against blank images, then a real one)
    assert all(r["img_align_n_tracked"] > 30 for r in hip[30:34])
    Tr = np.stack([r["T_f_w"] for r in ref])
    Th = np.stack([r["T_f_w"] for r in hip])
    d = se3.log_norm(Th, Tr)
    print(f"relocalization sequence: SE3 log-norm max {d.max():.3e} median {np.median(d):.3e}; stages {st_hip[28:36]}")
    assert d.max() <= SE3_LOGNORM_TOL


@pytest.mark.gpu
def test_dropin_second_sequence_with_noise(pipeline_libs, gpu_device):
    cam, imgs, T = _sequence(80, seed=11)
    rng = np.random.default_rng(3)
    imgs = np.clip(imgs.astype(np.float32) + rng.normal(0, 2.0, imgs.shape), 0, 255).round().astype(np.uint8)
    ref = pp.run_sequence("ref", cam, imgs, T)
    hip = pp.run_sequence("hip", cam, imgs, T)
    Tr = np.stack([r["T_f_w"] for r in ref])
    Th = np.stack([r["T_f_w"] for r in hip])
    d = se3.log_norm(Th, Tr)
    print(f"noisy sequence: SE3 log-norm max {d.max():.3e} median {np.median(d):.3e}")
    assert d.max() <= SE3_LOGNORM_TOL_NOISY and np.median(d) <= 1e-6
    assert [r["is_keyframe"] for r in ref] == [r["is_keyframe"] for r in hip]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["atan", "radtan"])
def test_dropin_sequence_with_the_reference_launch_file_cameras(pipeline_libs, gpu_device, kind):
    """The cameras SVO's own launch files configure (svo_ros/param/camera_atan.yaml: vk::ATANCamera,
    camera_pinhole.yaml: vk::PinholeCamera with radial-tangential distortion).  The drop-in recovers
    the model and its parameters through vk::AbstractCamera::world2cam (marshal.h) and runs every
    kernel with it; same comparison as the pinhole sequence."""
    from helpers import camera_models
    cam, imgs, T = _sequence(80, seed=7, cam=camera_models()[kind])
    ref = pp.run_sequence("ref", cam, imgs, T)
    hip = pp.run_sequence("hip", cam, imgs, T)
    Tr = np.stack([r["T_f_w"] for r in ref])
    Th = np.stack([r["T_f_w"] for r in hip])
    d = se3.log_norm(Th, Tr)
    print(f"{kind} camera: SE3 log-norm max {d.max():.3e} median {np.median(d):.3e}; keyframes {sum(r['is_keyframe'] for r in ref)}")
    assert all(r["stage"] == pp.STAGE_DEFAULT_FRAME for r in hip)
    assert [r["is_keyframe"] for r in ref] == [r["is_keyframe"] for r in hip]
    # Until the first depth-filter points enter the map (second keyframe) every stage sees the same
    # map: the camera model is exercised by every kernel and the poses agree like the pinhole ones.
    kf2 = [i for i, r in enumerate(ref) if r["is_keyframe"]][1]
    assert d[:kf2 + 1].max() <= SE3_LOGNORM_TOL and np.median(d[:kf2 + 1]) <= 1e-7, d[:kf2 + 1].max()
    # Afterwards the two maps differ by what a seed converging ONE update apart contributes (the float
    # test sqrt(sigma2) < z_range/200 flips on the last bit of an expf): a point created from mu_k in one
    # run and mu_k+1 in the other moves by a fraction of its sigma, and the poses follow at the 1e-5..1e-3
    # level -- for ANY camera model (scripts/dropin_camera_debug.py); both runs track the ground truth alike.
    assert np.median(d) <= 2e-4 and d.max() <= 5e-3
    err_h, err_r = se3.log_norm(Th, T), se3.log_norm(Tr, T)
    assert err_h.max() < 0.05 and abs(err_h.max() - err_r.max()) < 5e-3


@pytest.mark.gpu
def test_standalone_matcher_and_feature_alignment_seams(pipeline_libs, gpu_device):
    """Flavour "hipm": Reprojector, DepthFilter and FastDetector are the reference's own files and call
    svo::Matcher, which is the drop-in here (findMatchDirect / findEpipolarMatchDirect = one device trial
    per call, rpg_svo_amd/host/dropin/matcher.cpp) together with feature_alignment::align1D/align2D
    (dropin/feature_alignment.cpp): the seams of matcher.h:106-123 and feature_alignment.h:29-44 used the
    way a direct caller uses them."""
    if not pp.available("hipm"):
        pytest.skip("tests/dropin/_build/libsvo_pipeline_hipm.so not built")
    cam, imgs, T = _sequence(45, seed=5)
    ref = pp.run_sequence("ref", cam, imgs, T)
    hip = pp.run_sequence("hipm", cam, imgs, T)
    Tr = np.stack([r["T_f_w"] for r in ref])
    Th = np.stack([r["T_f_w"] for r in hip])
    d = se3.log_norm(Th, Tr)
    print(f"stand-alone seams: SE3 log-norm max {d.max():.3e} median {np.median(d):.3e}")
    assert all(r["stage"] == pp.STAGE_DEFAULT_FRAME for r in hip)
    assert d.max() <= SE3_LOGNORM_TOL and np.median(d) <= 1e-6
    assert [r["is_keyframe"] for r in ref] == [r["is_keyframe"] for r in hip]
    for k in ("repr_n_mps", "repr_n_new_references", "sfba_n_edges_final", "img_align_n_tracked"):
        assert np.mean([a[k] == b[k] for a, b in zip(ref, hip)]) >= 0.95, k
    assert np.mean([abs(a["n_seeds"] - b["n_seeds"]) <= 2 for a, b in zip(ref, hip)]) >= 0.95


@pytest.mark.gpu
def test_dropin_with_asynchronous_mapper_thread(pipeline_libs, gpu_device):
    """DepthFilter's own thread left running (the reference's normal mode): tracking lane and
    mapping lane of svo_hip::Device work concurrently.  Interleaving is timing dependent -- as in
    the reference -- so the check is against ground truth, not frame-by-frame equality."""
    cam, imgs, T = _sequence(120)
    for _ in range(2):
        hip = pp.run_sequence("hip", cam, imgs, T, mapper_thread=1)
        est = np.stack([r["T_f_w"] for r in hip])
        assert all(r["stage"] == pp.STAGE_DEFAULT_FRAME for r in hip)
        assert se3.log_norm(est, T).max() < 5e-3
        assert sum(r["is_keyframe"] for r in hip) >= 3
        assert max(r["n_candidates"] for r in hip) > 50


@pytest.mark.gpu
def test_dropin_deferred_mapper_is_the_synchronous_one(pipeline_libs, gpu_device):
    """svo_hip::Device::setDeferredMapping(true): DepthFilter::updateSeeds returns with its kernels running and its
    results reach the seed list / the map at the next reprojectMap, updateSeeds or detect.  Every consumer sees what the
    synchronous filter would have left, so the trajectory is IDENTICAL; only the harness' own read-out of the seed and
    candidate counts (taken right after addImage) lags by that one update."""
    cam, imgs, T = _sequence(120)
    a_st, b_st = {}, {}
    a = pp.run_sequence("hip", cam, imgs, T, stats_out=a_st)
    b = pp.run_sequence("hip", cam, imgs, T, stats_out=b_st, defer_mapper=1)
    assert np.array_equal(np.stack([r["T_f_w"] for r in a]), np.stack([r["T_f_w"] for r in b]))
    for k in ("is_keyframe", "n_obs", "repr_n_mps", "repr_n_new_references", "n_kfs", "stage"):
        assert [r[k] for r in a] == [r[k] for r in b], k
    assert a[-1]["n_seeds"] > 0 and sum(r["n_candidates"] for r in b) > 0
    ta, tb = (np.median([r["t_tot_time"] for r in x[1:]]) * 1e3 for x in (a, b))
    print(f"addImage median {ta:.3f} ms synchronous, {tb:.3f} ms with the mapper deferred; frame period "
          f"{a_st['wall_ms_per_frame']:.3f} / {b_st['wall_ms_per_frame']:.3f} ms")
    # a second sequence in the same process after a deferred one: nothing pending leaks across handlers
    c = pp.run_sequence("hip", cam, imgs[:30], T[:30])
    assert np.array_equal(np.stack([r["T_f_w"] for r in c]), np.stack([r["T_f_w"] for r in a[:30]]))


@pytest.mark.gpu
def test_dropin_small_pyramid_pool_evicts_and_reuploads(pipeline_libs, gpu_device):
    """A device pool of 7 pyramid slots for a run that keeps up to 5 keyframes + 2 working frames
    alive: live frames get evicted (LRU) and uploaded again on their next use; the trajectory
    must not notice."""
    cam, imgs, T = _sequence(120)
    big, small = {}, {}
    ref = pp.run_sequence("hip", cam, imgs, T, stats_out=big, pool_slots=256)
    hip = pp.run_sequence("hip", cam, imgs, T, stats_out=small, pool_slots=7)
    assert big["evictions"] == 0 and big["uploads"] == len(imgs)
    assert small["evictions"] > 100 and small["uploads"] >= big["uploads"]
    a = np.stack([r["T_f_w"] for r in ref])
    b = np.stack([r["T_f_w"] for r in hip])
    assert np.array_equal(a, b)  # same kernels on the same bytes: identical, not just close


@pytest.mark.gpu
def test_two_cameras_of_different_geometry_in_one_process(pipeline_libs, gpu_device):
    """A heterogeneous rig: two FrameHandlerMono instances (752x480 and 640x480) fed alternately.
    Each image geometry gets its own device context (pyramid store layout); both must track."""
    cam_a, imgs_a, T_a = _sequence(40)
    cam_b = synth.Camera(640, 480, 400.0, 400.0, 320.0, 240.0)
    T_b = synth.make_trajectory(40, seed=9, max_step=0.02, max_rot_deg=0.3)
    imgs_b = synth.render(synth.make_texture(seed=12345), T_b, cam_b).numpy()
    pa, pb = pp.Pipeline("hip", cam_a), pp.Pipeline("hip", cam_b)
    try:
        pa.set_first_frame(imgs_a[0], 0.0, T_a[0], pp.range_map(cam_a, T_a[0]))
        pb.set_first_frame(imgs_b[0], 0.0, T_b[0], pp.range_map(cam_b, T_b[0]))
        for i in range(1, 40):
            ra = pa.add_image(imgs_a[i], float(i))
            rb = pb.add_image(imgs_b[i], float(i))
            assert ra["stage"] == pp.STAGE_DEFAULT_FRAME and rb["stage"] == pp.STAGE_DEFAULT_FRAME
            assert se3.log_norm(ra["T_f_w"][None], T_a[i][None])[0] < 5e-3
            assert se3.log_norm(rb["T_f_w"][None], T_b[i][None])[0] < 5e-3
    finally:
        pa.close()
        pb.close()


@pytest.mark.gpu
def test_dropin_without_prediction_follows_the_predicting_one(pipeline_libs, gpu_device, tmp_path):
    """SVO_HIP_SPECULATE=0 (pose refinement as a call of its own, observations marshalled by the host) against the
    default (enqueued by the reprojector, observations gathered on the device): the same optimizer on the same
    observations up to the summation order of a wave with a different number of observations per lane."""
    import subprocess
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {HERE!r}); sys.path.insert(0, {os.path.join(HERE, 'dropin')!r})\n"
        "import pypipeline as pp\n"
        "import test_dropin_pipeline as t\n"
        "cam, imgs, T = t._sequence(60)\n"
        "st = {}\n"
        "hip = pp.run_sequence('hip', cam, imgs, T, stats_out=st)\n"
        "np.save(sys.argv[1], np.stack([r['T_f_w'] for r in hip]))\n"
        "print(st['predicted_pose_hits'], st['predicted_pose_misses'])\n")
    out, hits = {}, {}
    for mode in ("1", "0"):
        path = str(tmp_path / f"traj_{mode}.npy")
        p = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, SVO_HIP_SPECULATE=mode), capture_output=True,
                           text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        out[mode] = np.load(path)
        hits[mode] = [int(x) for x in p.stdout.split()[-2:]]
    assert hits["1"] == [59, 0] and hits["0"] == [0, 0]
    d = se3.log_norm(out["0"], out["1"])
    assert d.max() <= SE3_LOGNORM_TOL, d.max()


@pytest.mark.gpu
def test_dropin_arena_modes_agree(pipeline_libs, gpu_device, tmp_path):
    """SVO_HIP_ARENA=hybrid (the default: inputs mirrored in HBM, results written by the kernels straight into the pinned
    host arena, the host polling the selection kernel's signal instead of waiting for the stream), =mirrored (every block
    copied both ways, prediction on a second stream) and =mapped (no copy commands at all): the same kernels on the same
    bytes.  The mode is fixed when a lane is created, hence one process each."""
    import subprocess
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {HERE!r}); sys.path.insert(0, {os.path.join(HERE, 'dropin')!r})\n"
        "import pypipeline as pp\n"
        "import test_dropin_pipeline as t\n"
        "cam, imgs, T = t._sequence(40)\n"
        "hip = pp.run_sequence('hip', cam, imgs, T)\n"
        "np.save(sys.argv[1], np.stack([r['T_f_w'] for r in hip]))\n")
    out = {}
    for mode in ("hybrid", "mirrored", "mapped"):
        path = str(tmp_path / f"traj_{mode}.npy")
        p = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, SVO_HIP_ARENA=mode), capture_output=True,
                           text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        out[mode] = np.load(path)
    for mode in ("mirrored", "mapped"):
        d = se3.log_norm(out[mode], out["hybrid"])
        assert d.max() <= SE3_LOGNORM_TOL, (mode, d.max())


def _seed_store_on_and_off(flavour, n, tmp_path):
    """the same sequence with the resident seed store (default) and with the list flattened per call, keyframes being
    inserted AND removed (max_n_kfs = 4: removeKeyframe erases a keyframe's seeds behind the store's back), plus the deferred
    mapper (the replay's erasures reach the store one call later)"""
    on, s_on = _run_mirror(flavour, n, {}, tmp_path, "store_on", max_n_kfs=4)
    off, s_off = _run_mirror(flavour, n, {"SVO_HIP_SEED_STORE": "off"}, tmp_path, "store_off", max_n_kfs=4)
    assert np.array_equal(on, off)                                   # same trajectory, bit for bit
    assert s_on["seeds"] == s_off["seeds"] and s_on["counts"] == s_off["counts"]
    st = s_on["seed_store"]
    assert s_off["seed_store"]["calls"] == 0 and st["calls"] > n // 2
    assert s_on["kfs"] >= 6                                          # more keyframes than the map holds: seeds were removed with them
    # a seed's record travels once: what was sent is the seeds ever created (plus at most the one full re-send of a grown store),
    # not seeds x calls
    created = sum(max(0, b - a) for a, b in zip(s_on["seeds"], s_on["seeds"][1:])) + s_on["seeds"][0]
    assert st["seed_records_sent"] <= 2 * created + 1024 and st["seed_records_sent"] * 8 < sum(s_on["seeds"]), (st, created)
    dfr, s_dfr = _run_mirror(flavour, n, {}, tmp_path, "store_deferred", max_n_kfs=4, defer_mapper=1)
    # (the synchronous mapper's update is enqueued by the pose optimizer's drop-in -- EarlyUpdate in dropin/depth_filter.cpp --
    # and dropped when the frame becomes a keyframe: those launches are calls the deferred mapper, which enqueues when the
    # reference calls, does not make)
    assert np.array_equal(dfr, on) and s_dfr["seed_store"]["calls"] == st["calls"] - s_on["early_dropped"]
    assert s_dfr["early_taken"] == 0 and s_dfr["early_dropped"] == 0 and s_on["early_taken"] > n // 2
    # (nearly all of them in two phases: the tables marshalled and uploaded before the pose optimizer's result had arrived)
    assert s_on["early_two_phase"] >= s_on["early_taken"] - 4, s_on["early_two_phase"]
    # ... and SVO_HIP_EARLY_MAPPER=0 (the update enqueued when the reference calls it, as up to round 5): the same frames
    late, s_late = _run_mirror(flavour, n, {"SVO_HIP_EARLY_MAPPER": "0"}, tmp_path, "store_late", max_n_kfs=4)
    assert np.array_equal(late, on) and s_late["seeds"] == s_on["seeds"] and s_late["early_taken"] == 0
    assert s_late["seed_store"]["calls"] == s_dfr["seed_store"]["calls"]
    print(f"early mapper [{flavour}]: taken {s_on['early_taken']} ({s_on['early_two_phase']} launched in two phases), dropped {s_on['early_dropped']} of {n - 1} frames")
    # SVO_HIP_SEED_STORE=verify (the host's state of every resident seed compared with what the device last reported, Seed::id
    # checked for monotonicity): nothing edits the seeds behind the store's back here, so nothing is re-sent
    ver, s_ver = _run_mirror(flavour, n, {"SVO_HIP_SEED_STORE": "verify"}, tmp_path, "store_verify", max_n_kfs=4)
    assert np.array_equal(ver, on) and s_ver["seed_store"]["seed_records_sent"] == st["seed_records_sent"]


def _frame_chain_on_and_off(flavour, n, tmp_path):
    """VERDICT r05 "one completion per frame" (rpg_svo_amd/host/dropin/frame_chain.h): reprojection, matching, selection and
    the predicted pose refinement of a frame enqueued BEHIND its sparse alignment, on the overlapping keyframes the prior
    pose finds and the pose the device composes from K1's result; reprojectMap verifies both against what the host
    computes and takes the batch.  Against SVO_HIP_CHAIN=0 (every step a call of its own, as up to round 5): bit-identical
    trajectories, the same trials / matches / projected points in every frame; the chain is taken on (nearly) every
    frame after the first reprojection -- a miss is a frame on which the final pose ranks the keyframes differently."""
    kw = dict(max_n_kfs=4)
    on, s_on = _run_mirror(flavour, n, {"SVO_HIP_MAP_MIRROR": "verify"}, tmp_path, "chain_on", **kw)
    off, s_off = _run_mirror(flavour, n, {"SVO_HIP_MAP_MIRROR": "verify", "SVO_HIP_CHAIN": "0"}, tmp_path, "chain_off", **kw)
    assert np.array_equal(on, off)
    assert s_on["counts"] == s_off["counts"] and s_on["seeds"] == s_off["seeds"]
    assert s_off["chain_hits"] == 0 and s_off["chain_misses"] == 0
    print(f"frame chain [{flavour}]: taken {s_on['chain_hits']}, not taken {s_on['chain_misses']} of {n - 1} frames; "
          f"pose refinements predicted {s_on['hits']}")
    assert s_on["chain_hits"] >= 0.9 * (n - 2) and s_on["chain_hits"] + s_on["chain_misses"] <= n - 2
    assert s_on["hits"] == s_off["hits"] == n - 1 and s_on["fallbacks"] == 0 and s_on["kfs"] >= 5
    # the deferred mapper (its results are written back before the chain reads the map) and the mapper thread
    dfr, s_dfr = _run_mirror(flavour, n, {"SVO_HIP_MAP_MIRROR": "verify"}, tmp_path, "chain_deferred", defer_mapper=1, **kw)
    assert np.array_equal(dfr, on) and s_dfr["chain_hits"] == s_on["chain_hits"]
    _, s_thr = _run_mirror(flavour, 100, {"SVO_HIP_MAP_MIRROR": "verify"}, tmp_path, "chain_thr", mapper_thread=1)
    assert s_thr["fallbacks"] == 0 and s_thr["chain_hits"] + s_thr["chain_misses"] <= 98
    # without the predicted pose refinement the chain ends with the match kernels
    nop, s_nop = _run_mirror(flavour, 60, {"SVO_HIP_SPECULATE": "0"}, tmp_path, "chain_nopred")
    ref60, _ = _run_mirror(flavour, 60, {"SVO_HIP_SPECULATE": "0", "SVO_HIP_CHAIN": "0"}, tmp_path, "chain_nopred_off")
    assert np.array_equal(nop, ref60) and s_nop["chain_hits"] >= 50 and s_nop["hits"] == 0


def test_mock_device_frame_chain_behind_the_sparse_alignment(mock_lib, tmp_path):
    _frame_chain_on_and_off("hipmock", 160, tmp_path)


@pytest.mark.gpu
def test_dropin_frame_chain_behind_the_sparse_alignment_on_the_gpu(pipeline_libs, gpu_device, tmp_path):
    _frame_chain_on_and_off("hip", 160, tmp_path)


def test_mock_device_resident_seed_store_is_the_flattened_list(mock_lib, tmp_path):
    """Row N2, seeds, host side (rpg_svo_amd/host/dropin/seed_store.h) on the mock device."""
    _seed_store_on_and_off("hipmock", 200, tmp_path)


FAULT_CODE = (
    "import sys, numpy as np\n"
    "sys.path.insert(0, {here!r}); sys.path.insert(0, {dropin!r})\n"
    "import pypipeline as pp\n"
    "import test_dropin_pipeline as t\n"
    "cam, imgs, T = t._sequence(80)\n"
    "p = pp.Pipeline('hipmock', cam, max_n_kfs=4)\n"
    "p.set_first_frame(imgs[0], 0.0, T[0], pp.range_map(cam, T[0]))\n"
    "out, threw = [], []\n"
    "for i in range(1, len(imgs)):\n"
    "    try:\n"
    "        out.append(p.add_image(imgs[i], float(i))['T_f_w'])\n"
    "    except RuntimeError as e:\n"
    "        threw.append(i); out.append(np.zeros(12))\n"
    "np.save(sys.argv[1], np.stack(out))\n"
    "print(threw, list(p.seed_store_stats()))\n")


def test_mock_device_seed_store_forgets_what_a_failed_call_left_behind(mock_lib, tmp_path):
    """SeedStore::sync() commits its shadow before the patch kernel is enqueued.  The mock fails the
    second svo_hip_seed_store_patch (the records of a keyframe's new seeds never reach the store): updateSeeds throws, the
    store must forget its shadow (SeedStore::invalidate) and re-send the whole list with the next call -- the frames after
    the failure are then, bit for bit, those of the flattened-list path whose update fails at the same frame.  (Without the
    invalidation the next update reads slots that were never written and a garbage frame index.)"""
    import subprocess
    code = FAULT_CODE.format(here=HERE, dropin=os.path.join(HERE, "dropin"))

    def run(tag, env):
        path = str(tmp_path / f"fault_{tag}.npy")
        p = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        threw, stats = eval(p.stdout.strip().splitlines()[-1].replace("] [", "], ["))
        return np.load(path), threw, stats

    on, threw_on, st_on = run("on", {"SVO_MOCK_FAIL_SEED_PATCH_AT": "2"})
    assert len(threw_on) == 1, threw_on
    # the store-off path makes one svo_hip_update_seeds call per updateSeeds: find the call of the same frame
    probe, threw_p, _ = run("probe", {"SVO_HIP_SEED_STORE": "off", "SVO_MOCK_FAIL_UPDATE_SEEDS_AT": "1"})
    # (a failed first update shifts the later calls by a frame or so: try the neighbours of the estimate)
    for k in (threw_on[0] - threw_p[0], 1 + threw_on[0] - threw_p[0], 2 + threw_on[0] - threw_p[0]):
        off, threw_off, st_off = run("off", {"SVO_HIP_SEED_STORE": "off", "SVO_MOCK_FAIL_UPDATE_SEEDS_AT": str(k)})
        if threw_off == threw_on:
            break
    assert threw_off == threw_on, (threw_off, threw_on)
    assert np.array_equal(on, off)
    assert st_off[0] == 0 and st_on[0] > 40


@pytest.mark.gpu
def test_dropin_resident_seed_store_is_the_flattened_list_on_the_gpu(pipeline_libs, gpu_device, tmp_path):
    """The same on the real device: svo_hip_seed_store_patch + svo_hip_update_seeds_resident against svo_hip_update_seeds."""
    _seed_store_on_and_off("hip", 160, tmp_path)


@pytest.mark.gpu
def test_dropin_map_mirror_is_the_list_walk_on_the_gpu(pipeline_libs, gpu_device, tmp_path):
    """The same on the real device: svo_hip_reproject_map + the indirect match batch against the list-walking path that
    marshals every trial on the host -- same kernels on the same trials, so the trajectories are equal bit for bit; verify
    mode holds over keyframe insertions and removals."""
    n = 160
    off, s_off = _run_mirror("hip", n, {"SVO_HIP_MAP_MIRROR": "off"}, tmp_path, "off", max_n_kfs=4)
    ver, s_ver = _run_mirror("hip", n, {"SVO_HIP_MAP_MIRROR": "verify"}, tmp_path, "verify", max_n_kfs=4)
    assert np.array_equal(ver, off)
    assert s_ver["counts"] == s_off["counts"]
    assert s_ver["calls"] == n - 1 and s_ver["fallbacks"] == 0 and s_ver["hits"] == n - 1 and s_ver["kfs"] >= 5
    # the depth filter on its own thread (its kernels on the mapping lane's stream, candidates appended to the map while the
    # tracker runs): verify holds, no frame leaves the mirror
    _, s_thr = _run_mirror("hip", 100, {"SVO_HIP_MAP_MIRROR": "verify"}, tmp_path, "thr", mapper_thread=1)
    assert s_thr["calls"] == 99 and s_thr["fallbacks"] == 0
