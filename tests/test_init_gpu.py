"""The whole two-view bootstrap on the device: rpg_svo_amd.initialization.KltHomographyInit on a rendered scene of
tests/klt_scenes.py (a textured plane seen along a random walk, 5-level store), frame after frame as
FrameHandlerMono::processFirstFrame / processSecondFrame call it.  NO_KEYFRAME until the median disparity passes 50 px,
then SUCCESS with at least initMinInliers inliers; H transfers the renderer's true positions of the inliers to within
1 px; the median depth of the new points in the current frame is mapScale; and, when the decomposition is not flagged
ambiguous, the pose matches the renderer's up to scale within the caps of tests/test_homography_checker.py's noisy case
(rotation 2e-2 rad, translation direction 0.1 rad).  A pure plane is ambiguous in the reference's own algorithm about
40 % of the time: then only the H-level and inlier conditions apply."""
import numpy as np
import pytest
import torch

import homography_cases as cases
import klt_scenes
from rpg_svo_amd import synth
from test_klt_gpu import make_store

pytestmark = pytest.mark.gpu

MAP_SCALE = 1.5


def test_two_images_to_a_scaled_pose_and_a_point_cloud(gpu_device):
    from rpg_svo_amd.initialization import InitResult, KltHomographyInit
    seed, max_step, n_frames = klt_scenes.SCENES[3]
    s = klt_scenes.make_scene(seed, max_step, n_frames)
    flat = np.full_like(s.images, 127)
    store = make_store(np.concatenate([s.images, flat]), gpu_device)
    slots = lambda k: torch.tensor([k, n_frames + k], dtype=torch.int32, device=gpu_device)
    init = KltHomographyInit(s.cam, homography=dict(map_scale=MAP_SCALE))
    T0 = torch.from_numpy(np.stack([s.T[0], s.T[0]])).to(gpu_device)
    first = init.add_first_frame(store, slots(0), T0).cpu().numpy()
    assert list(first) == [InitResult.SUCCESS, InitResult.FAILURE]
    valid = init.status[0].cpu().numpy() != 0
    px_ref = init.px_ref[0].cpu().numpy().astype(np.float64)
    _, X = synth.features_3d(s.T[:1], s.cam, torch.from_numpy(px_ref[None]))
    X = X[0].numpy()
    done = False
    for k in range(1, n_frames):
        res = init.add_second_frame(store, slots(k)).cpu().numpy()
        med, n_tracked = float(init.median_disparity[0].item()), int(init.n_tracked[0].item())
        print(f"frame {k}: {InitResult(int(res[0])).name}, tracked {n_tracked}, median disparity {med:.2f} px")
        assert res[1] == InitResult.FAILURE and int(init.out["status"][1].item()) == 1 and not bool(init.points[1].any())
        if med < 50.0:
            assert res[0] == InitResult.NO_KEYFRAME and int(init.n_inliers[0].item()) == 0 and not bool(init.points[0].any())
            continue
        assert res[0] == InitResult.SUCCESS
        done = True
        break
    assert done
    get = lambda t: t[0].cpu().numpy()
    inl, ok, amb = get(init.inliers) != 0, get(init.point_ok) != 0, int(get(init.ambiguous))
    n_inl = int(get(init.n_inliers))
    tracked = get(init.status) != 0
    assert n_inl == inl.sum() >= init.homography_params.min_inliers and not inl[~tracked].any() and not ok[~inl].any()
    # H against the renderer
    H = get(init.H).reshape(3, 3)
    truth = synth._proj(s.T[k], s.cam, X)[0]
    uv = np.stack([(px_ref[:, 0] - s.cam.cx) / s.cam.fx, (px_ref[:, 1] - s.cam.cy) / s.cam.fy, np.ones(len(px_ref))], axis=1)
    y = uv[inl] @ H.T
    pred = np.stack([s.cam.fx * y[:, 0] / y[:, 2] + s.cam.cx, s.cam.fy * y[:, 1] / y[:, 2] + s.cam.cy], axis=1)
    off = np.linalg.norm(pred - truth[inl], axis=1)
    print(f"H against the renderer over {n_inl} inliers: median {np.median(off):.3f} px, max {off.max():.3f} px; ambiguous {amb}")
    assert off.max() <= 1.0
    # the scale fix: the median depth of the new points in the current frame is mapScale
    T = get(init.T_f_w)
    R_cw, t_cw = T[:9].reshape(3, 3), T[9:]
    P = get(init.points)
    z = np.sort((P[inl] @ R_cw.T + t_cw)[:, 2])
    print(f"median depth of the map points in the current frame {z[len(z) // 2]:.15f} (mapScale {MAP_SCALE}), scale {float(get(init.scale)):.6f}")
    assert abs(z[len(z) // 2] - MAP_SCALE) <= 1e-9 * MAP_SCALE
    assert (z[ok[inl]] > 0).all() and ok.any() and not P[~inl].any()
    # the pose against the renderer's, up to scale
    Rt = lambda T12: (T12[:9].reshape(3, 3), T12[9:])
    R0, t0 = Rt(s.T[0])
    Rk, tk = Rt(s.T[k])
    R_true, t_true = Rk @ R0.T, tk - Rk @ R0.T @ t0
    Tcr = get(init.T_cur_from_ref)
    rot, tra = cases.rotation_angle(Tcr[:9].reshape(3, 3), R_true), cases.direction_angle(Tcr[9:], t_true)
    print(f"pose against the renderer: rotation {rot:.2e} rad, translation direction {tra:.2e} rad")
    if not amb:
        assert rot <= 2e-2 and tra <= 0.1
        assert cases.rotation_angle(R_cw, Rk) <= 2e-2
