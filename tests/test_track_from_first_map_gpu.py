"""From the first map through one tracked frame to the next frame's K1 inputs and a keyframe decision, without a host read in
between: the scene and the bootstrap of tests/test_bootstrap_to_tracking_gpu.py (SUCCESS at frame 8 of 10; sequence 1 is a
flat image that failed), then rpg_svo_amd.tracking.track_from_first_map on frame 9: K1, compose_poses, reproject_points,
find_match_direct with two observation records per point, select_matches, optimize_gauss_newton, close_frame.

The test asserts, and prints the figures of:
 1. close_frame's outputs equal the checker (tests/frame_close_checker.py) run on the downloaded inputs of that call, by the
    rule of first_map_cases.compare_device (discrete outputs equal, f64 within 1e-14 relative); sequence 1 leaves by gate 1
    with T_out == T_last;
 2. the result of sequence 0 is not RESULT_FAILURE, and the rotation of its tracked pose against the renderer's (frame 8 ->
    frame 9) is within 2e-2 rad unless K9 flagged the pair ambiguous (the cap of tests/test_init_gpu.py);
 3. SparseImgAlign(4, 2).run with reference slot 9, current slot 8 and an identity prior, fed with close_frame's px /
    xyz_ref / valid as they are, gives the same n_tracked as the same call fed by marshal_problem on the downloaded features,
    and a pose within 1e-6 SE(3) log-norm of it.

Measured on an MI355X: sequence 0 has 260 trials, 260 matched, 121 features, 121 edges after pruning (last frame 263); gate 0,
quality TRACKING_GOOD, depth_mean 1.495343, depth_min 1.481056, kf_block 0, result NO_KEYFRAME, nobs_out 121; sequence 1: no
trial, gate 1, FAILURE; largest difference of close_frame to the checker 0; rotation against the renderer's 1.31e-4 rad,
ambiguous 0; K1 tracks 120 patches from either input, the two poses 0 apart (xyz_ref against numpy's norm 5.7e-16 relative)."""
import numpy as np
import pytest
import torch

import frame_close_cases as cases
import frame_close_checker as chk
from first_map_cases import compare_device
from host_buffers import relative_difference, same_bits
from test_bootstrap_to_tracking_gpu import bootstrap

pytestmark = pytest.mark.gpu


def test_a_tracked_frame_from_the_first_map(gpu_device):
    from homography_cases import rotation_angle
    from rpg_svo_amd import capi, se3, tracking as tr
    from rpg_svo_amd.map_mirror import Grid
    from rpg_svo_amd.sparse_img_align import SparseImgAlign, marshal_problem
    dev = gpu_device
    s, store, slots, init, k, _ = bootstrap(dev)
    nxt = k + 1
    assert nxt < len(s.T)
    fm = init.first_map(store, slots(k), batch_id=1)
    det = init.detector
    det_grid = (det.cell_size, det.grid_n_cols, det.grid_n_rows)
    n_cols, n_rows = -(-s.cam.width // 30), -(-s.cam.height // 30)
    grid = Grid.for_camera(s.cam.width, s.cam.height, 30, np.random.default_rng(5).permutation(n_cols * n_rows), dev)
    kf_T = (init.T_ref_w, init.T_f_w.contiguous())
    tf = tr.track_from_first_map(store, s.cam, fm, (slots(0), slots(k)), kf_T, slots(nxt), grid, det_grid)
    torch.cuda.synchronize()
    get = lambda t: t.cpu().numpy()
    ambiguous = int(get(init.ambiguous)[0])

    # 1. the checker on the downloaded inputs of the call
    n = 2
    inp = dict(n=get(tf.n_matches), px=get(tf.px), f=get(tf.f), pos=get(tf.pos), has_point=get(tf.pose.has_point), T_f_w=get(tf.pose.T_f_w),
               T_last=get(kf_T[1]), num_obs=get(tf.num_obs), num_obs_last=get(fm.n_points), n_kf=np.full(n, 2, np.int32),
               kf_T=np.stack([get(kf_T[0]), get(kf_T[1])], axis=1), kf_overlap=np.zeros((n, 2), np.int32))
    want = chk.frame_close(s.cam, inp, *det_grid)
    got = {name: get(getattr(tf.close, name)) for name in cases.out_shapes(1, 1, 1)}
    worst, _ = compare_device(got, want, cases.DISCRETE, cases.CONTINUOUS, what="close_frame")
    names = {capi.RESULT_NO_KEYFRAME: "NO_KEYFRAME", capi.RESULT_IS_KEYFRAME: "IS_KEYFRAME", capi.RESULT_FAILURE: "FAILURE"}
    for b in range(n):
        print(f"sequence {b}: {int(get(tf.n_trials)[b])} trials, {int((get(tf.match.ok).reshape(n, -1)[b] > 0).sum())} matched, "
              f"{int(inp['n'][b])} features, {int(inp['num_obs'][b])} edges after pruning (last frame {int(inp['num_obs_last'][b])}); gate "
              f"{int(got['gate'][b])}, quality {int(got['quality'][b])}, depth_mean {got['depth_mean'][b]:.6f}, depth_min {got['depth_min'][b]:.6f}, "
              f"kf_block {int(got['kf_block'][b])}, result {names[int(got['result'][b])]}, nobs_out {int(got['nobs_out'][b])}")
    print(f"largest relative difference of close_frame to the checker {worst:.2e}")
    assert got["gate"][1] == 1 and got["result"][1] == capi.RESULT_FAILURE and same_bits(got["T_out"][1], inp["T_last"][1])
    assert inp["n"][1] == 0 and got["nobs_out"][1] == 0

    # 2. sequence 0 tracked, and its rotation against the renderer's
    assert got["result"][0] != capi.RESULT_FAILURE and got["gate"][0] == 0
    R = lambda T12: np.asarray(T12)[:9].reshape(3, 3)
    rot = rotation_angle(R(got["T_out"][0]) @ R(inp["T_last"][0]).T, R(s.T[nxt]) @ R(s.T[k]).T)
    print(f"rotation of the tracked pose (frame {k} -> frame {nxt}) against the renderer's: {rot:.2e} rad; ambiguous {ambiguous}")
    if not ambiguous:
        assert rot <= 2e-2

    # 3. K1 on close_frame's outputs as they are, against K1 on the host-marshalled features
    sia = SparseImgAlign(4, 2)
    one = lambda t: t[0:1].contiguous()
    ref_slot, cur_slot = one(slots(nxt)), one(slots(k))
    prior = torch.tensor([[1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], dtype=torch.float64, device=dev)
    on_device = sia.run(store, s.cam, ref_slot, cur_slot, one(tf.n_matches), one(tf.px), one(tf.close.xyz_ref), prior, valid=one(tf.close.valid))
    hp = inp["has_point"][0] != 0
    hp[int(inp["n"][0]):] = False
    pos_host = np.where(hp[:, None], inp["pos"][0], 0.0)
    _, xyz_host = marshal_problem(got["T_out"][0], got["T_out"][0], inp["f"][0], pos_host)
    xyz_host[~hp] = 0.0
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    on_host = sia.run(store, s.cam, ref_slot, cur_slot, t(inp["n"][0:1], torch.int32), t(inp["px"][0:1], torch.float64),
                      t(xyz_host[None], torch.float64), prior, valid=t(hp[None].astype(np.uint8), torch.uint8))
    torch.cuda.synchronize()
    d = float(se3.log_norm(get(on_device.T_cur_from_ref), get(on_host.T_cur_from_ref)).max())
    depth_diff = relative_difference(got["xyz_ref"][0][hp], xyz_host[hp])
    print(f"K1 on the tracked frame: n_tracked {int(on_device.n_tracked[0])} (host-marshalled {int(on_host.n_tracked[0])}), SE(3) log-norm "
          f"between the two poses {d:.2e}; xyz_ref against numpy's norm {depth_diff:.2e} relative")
    assert np.array_equal(got["valid"][0] != 0, hp)
    assert int(on_device.n_tracked[0]) == int(on_host.n_tracked[0]) > 0
    assert d <= 1e-6
