"""From two images to a state that tracking runs on, without a host read in between: the scene of tests/test_init_gpu.py
(klt_scenes.SCENES[3]: a textured plane along a random walk, 5-level store) frame after frame up to SUCCESS at frame k,
then KltHomographyInit.first_map (svo_hip_first_map, FastDetector.detect on the free cells, svo_hip_initialize_seeds).

Checked on the CPU beforehand with the oracle's FAST, tests/klt_checker.py and tests/homography_checker.py: 319 corners;
the median disparity passes 50 px at frame k = 8 (48.23 px at frame 7, 56.18 px at frame 8, 272 points tracked); the
homography step gives SUCCESS there with 270 inliers, 263 of them map points, and `ambiguous` is 0.

The test asserts, and prints the figures of:
 1. the first map equals the checker (tests/first_map_checker.py) run on the downloaded K9 outputs, by the rule of
    first_map_cases.compare_device (discrete outputs equal, f64 within 1e-14 relative, f32 seed fields within 1 ulp);
 2. no seed lies in an occupied cell, and n_seeds is the number of free cells with a corner (the detector run once more
    without the occupancy);
 3. SparseImgAlign(4, 2).run with reference slot k, current slot k - 1 and an identity prior, fed with FirstMap.px[:, 1],
    xyz_ref and n_points as they are, gives the same n_tracked as the same call fed by marshal_problem on the downloaded
    map, and a pose within 1e-6 SE(3) log-norm of it;
 4. when K9 did not flag the pair ambiguous, that pose's rotation is within 2e-2 rad of the renderer's (the cap of
    tests/test_init_gpu.py).

Measured on an MI355X: SUCCESS at frame 8 (272 tracked, median disparity 56.18 px, as the CPU check says), 263 map points,
depth_mean 1.500300 (mapScale 1.5), depth_min 1.485263, largest difference to the checker 0 (seeds 0, 0 ulp); 130 seeds in
164 free cells of 352; K1 tracks 259 patches from either input and the two poses differ by 3.5e-18 in SE(3) log-norm
(xyz_ref differs from numpy's norm by 4.5e-16 relative); rotation against the renderer's 2.3e-4 rad, ambiguous 0."""
import numpy as np
import pytest
import torch

import first_map_cases as cases
import first_map_checker as chk
from host_buffers import relative_difference
import klt_scenes
from test_klt_gpu import make_store

pytestmark = pytest.mark.gpu

MAP_SCALE = 1.5


def bootstrap(dev):
    """The scene up to the frame that gives SUCCESS.  -> (scene, store, slots, init, k, (px_cur, status) before frame k);
    sequence 1 is a flat image that fails at the first frame."""
    from rpg_svo_amd.initialization import InitResult, KltHomographyInit
    seed, max_step, n_frames = klt_scenes.SCENES[3]
    s = klt_scenes.make_scene(seed, max_step, n_frames)
    store = make_store(np.concatenate([s.images, np.full_like(s.images, 127)]), dev)
    slots = lambda k: torch.tensor([k, n_frames + k], dtype=torch.int32, device=dev)
    init = KltHomographyInit(s.cam, homography=dict(map_scale=MAP_SCALE))
    T0 = torch.from_numpy(np.stack([s.T[0], s.T[0]])).to(dev)
    first = init.add_first_frame(store, slots(0), T0).cpu().numpy()
    assert list(first) == [InitResult.SUCCESS, InitResult.FAILURE]
    for k in range(1, n_frames):
        before = (init.px_cur.clone(), init.status.clone())
        res = init.add_second_frame(store, slots(k)).cpu().numpy()
        print(f"frame {k}: {InitResult(int(res[0])).name}, tracked {int(init.n_tracked[0])}, median disparity {float(init.median_disparity[0]):.2f} px")
        assert res[1] == InitResult.FAILURE
        if res[0] == InitResult.SUCCESS:
            return s, store, slots, init, k, before
        assert res[0] == InitResult.NO_KEYFRAME
    raise AssertionError("the scene never reached SUCCESS")


def test_two_images_to_a_state_that_tracking_runs_on(gpu_device):
    from rpg_svo_amd import se3
    from rpg_svo_amd.sparse_img_align import SparseImgAlign, marshal_problem
    dev = gpu_device
    s, store, slots, init, k, _ = bootstrap(dev)
    assert k >= 1
    fm = init.first_map(store, slots(k), batch_id=1)
    torch.cuda.synchronize()
    det = init.detector
    grid = (det.cell_size, det.grid_n_cols, det.grid_n_rows)
    get = lambda t: t.cpu().numpy()
    ambiguous = int(get(init.ambiguous)[0])

    # 1. the checker on the downloaded K9 outputs
    want = chk.first_map(s.cam, get(init.result), get(init.point_ok), get(init.points), get(init.px_ref), get(init.px_cur), get(init.f_ref),
                         get(init.f_cur), get(init.T_f_w), *grid)
    got = {n: get(getattr(fm, n)) for n in cases.out_shapes(1, 1, 1)}
    worst, _ = cases.compare_device(got, want, cases.DISCRETE, cases.CONTINUOUS, what="first map")
    n_points = int(got["n_points"][0])
    assert n_points == int(get(init.point_ok)[0].sum()) >= 40 and got["n_points"][1] == 0
    xy, level, score = (get(t) for t in det.detect(store, slots(k), init.min_corner_score, fm.occupancy))
    seeds_want = chk.initialize_seeds(s.cam, xy, level, score, init.min_corner_score, np.arange(2, dtype=np.int32), got["depth_mean"],
                                      0.5 * got["depth_min"], 1, det.n_cells)
    seeds_got = dict(n_seeds=fm.n_seeds, frame=fm.seed_ftr.frame, level=fm.seed_ftr.level, type=fm.seed_ftr.type, px=fm.seed_ftr.px, f=fm.seed_ftr.f,
                     grad=fm.seed_ftr.grad, a=fm.seeds.a, b=fm.seeds.b, mu=fm.seeds.mu, z_range=fm.seeds.z_range, sigma2=fm.seeds.sigma2,
                     batch_id=fm.seeds.batch_id)
    worst_seed, ulps = cases.compare_device({n: get(v) for n, v in seeds_got.items()}, seeds_want, cases.SEED_DISCRETE, cases.SEED_F64, cases.SEED_F32,
                                            what="seeds")
    print(f"first map: {n_points} points, key points {got['key_pts'][0].tolist()}, depth_mean {got['depth_mean'][0]:.6f}, depth_min "
          f"{got['depth_min'][0]:.6f}; largest relative difference to the checker {worst:.2e} (seeds {worst_seed:.2e}, f32 fields {ulps} ulp)")

    # 2. seeds only where the grid is free
    occ = got["occupancy"][0]
    n_seeds = int(get(fm.n_seeds)[0])
    px_seed = get(fm.seed_ftr.px)[0, :n_seeds]
    cell = (px_seed[:, 1] / det.cell_size).astype(int) * det.grid_n_cols + (px_seed[:, 0] / det.cell_size).astype(int)
    _, _, score_all = (get(t) for t in det.detect(store, slots(k), init.min_corner_score))
    free_with_corner = (score_all[0] > init.min_corner_score) & (occ == 0)
    print(f"seeds: {n_seeds} in {int((occ == 0).sum())} free cells of {det.n_cells} ({int(occ.sum())} occupied)")
    assert not occ[cell].any() and len(set(cell.tolist())) == n_seeds
    assert n_seeds == int(free_with_corner.sum()) > 0 and np.array_equal(np.sort(cell), np.flatnonzero(free_with_corner))

    # 3. K1 on that state as it is, against K1 on the host-marshalled map
    sia = SparseImgAlign(4, 2)
    one = lambda t: t[0:1].contiguous()
    ref_slot, cur_slot = slots(k)[0:1].contiguous(), slots(k - 1)[0:1].contiguous()
    prior = torch.tensor([[1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], dtype=torch.float64, device=dev)
    on_device = sia.run(store, s.cam, ref_slot, cur_slot, one(fm.n_points), fm.px[0:1, 1].contiguous(), one(fm.xyz_ref), prior)
    T_kw = get(init.T_f_w)[0]
    _, xyz_host = marshal_problem(T_kw, T_kw, got["f"][0, 1], got["pos"][0])
    xyz_host[n_points:] = 0.0
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    on_host = sia.run(store, s.cam, ref_slot, cur_slot, t([n_points], torch.int32), t(got["px"][0:1, 1], torch.float64),
                      t(xyz_host[None], torch.float64), prior)
    torch.cuda.synchronize()
    T_dev, T_host = get(on_device.T_cur_from_ref), get(on_host.T_cur_from_ref)
    d = float(se3.log_norm(T_dev, T_host).max())
    depth_diff = relative_difference(got["xyz_ref"][0, :n_points], xyz_host[:n_points])
    print(f"K1 on the first map: n_tracked {int(on_device.n_tracked[0])} (host-marshalled {int(on_host.n_tracked[0])}), SE(3) log-norm between "
          f"the two poses {d:.2e}; xyz_ref against numpy's norm {depth_diff:.2e} relative")
    assert int(on_device.n_tracked[0]) == int(on_host.n_tracked[0]) > 0
    assert d <= 1e-6

    # 4. the rotation against the renderer's (frame k -> frame k - 1)
    R = lambda T12: np.asarray(T12)[:9].reshape(3, 3)
    from homography_cases import rotation_angle
    rot = rotation_angle(R(T_dev[0]), R(s.T[k - 1]) @ R(s.T[k]).T)
    print(f"rotation of that pose against the renderer's: {rot:.2e} rad; ambiguous {ambiguous}")
    if not ambiguous:
        assert rot <= 2e-2
