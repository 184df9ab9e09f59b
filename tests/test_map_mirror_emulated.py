"""Row N2 without a GPU: rpg_svo_amd/csrc/map_mirror.hip compiled for the host through tests/host/hip_emu.h -- the C-ABI
entry point svo_hip_reproject_map itself, its one-workgroup kernel run by 1024 host threads (barriers, LDS, the scan's
__shfl_up, LDS atomics emulated) -- against the oracle's restatement of Reprojector::reprojectMap on random maps, exactly
as tests/test_map_mirror_gpu.py does on the device."""
import os

import numpy as np
import pytest

from helpers import camera_models, FUZZ, fuzz_rng, oracle_reproject_map, random_map
from map_mirror_host import compare, upload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[0], ids=["default"])
def emu(request):
    from emu_build import build_emulated
    from emu_build import BUILDS
    return build_emulated(BUILDS[request.param])


@pytest.mark.parametrize("kind", ["pinhole", "atan"])
def test_emulated_kernel_is_the_reference_walk(emu, oracle, kind):
    """Integer results (cells, counts, visiting order, trials, chosen observations) identical to the oracle; projections,
    host-compiled without contraction like the oracle, to 1e-12 px."""
    cam = camera_models()[kind]
    for seed, (n_points, n_cand) in enumerate([(900, 700), (2500, 1900), (40, 0), (0, 300), (0, 0)]):
        mp = random_map(cam, n_kfs=12, n_points=n_points, n_candidates=n_cand, seed=seed + 100 * FUZZ)
        m = upload(emu, mp)
        r = m.reproject(cam, mp["T"], mp["cur"], mp["kf_rank"], mp)
        V, M = compare(r, oracle_reproject_map(mp, cam), n_points + n_cand, 1e-12)
        if n_points + n_cand > 1000:
            assert V > 500 and 0 < M < V


def test_emulated_batches_and_patches(emu, oracle):
    cam = camera_models()["pinhole"]
    mp = random_map(cam, seed=11 + 100 * FUZZ)
    P = mp["pos"].shape[0]
    m = upload(emu, mp, capacity=P + 50)
    a = m.reproject(cam, mp["T"], mp["cur"], mp["kf_rank"], mp, max_cells_with_trials=40)
    oa = oracle_reproject_map(mp, cam, 0, 40)
    compare(a, oa, P, 1e-12)
    end = int(oa["header"][4])
    compare(m.reproject(cam, mp["T"], mp["cur"], mp["kf_rank"], mp, first_cell=end), oracle_reproject_map(mp, cam, end), P, 1e-12)
    # an incremental patch: positions move, types change, a new candidate with a new observation record is appended
    rng = fuzz_rng(5)
    idx = rng.choice(P, 60, replace=False)
    mp["pos"][idx] += rng.normal(0, 0.02, (60, 3))
    promoted = idx[mp["type"][idx] == 2][:5]
    mp["type"][promoted] = 3
    dead = idx[mp["type"][idx] != 0][-4:]
    mp["type"][dead] = 0
    O = mp["obs_frame"].shape[0]
    new_p = P
    mp["pos"] = np.vstack([mp["pos"], mp["pos"][idx[0]] + [0.05, 0.02, 0.0]])
    for k, v in (("type", 1), ("order", int(mp["order"].max()) + 1), ("obs_begin", O), ("obs_count", 1)):
        mp[k] = np.append(mp[k], v).astype(np.int32)
    for k, v in (("obs_frame", 3), ("obs_order", -1), ("obs_level", 1)):
        mp[k] = np.append(mp[k], v).astype(np.int32)
    mp["obs_type"] = np.append(mp["obs_type"], 0).astype(np.uint8)
    mp["obs_px"] = np.vstack([mp["obs_px"], [100.0, 120.0]])
    mp["obs_f"] = np.vstack([mp["obs_f"], [0.0, 0.0, 1.0]])
    mp["obs_grad"] = np.vstack([mp["obs_grad"], [1.0, 0.0]])
    touched = np.unique(np.concatenate([idx, [new_p]]))
    m.a["d_obs_frame"] = np.append(m.a["d_obs_frame"], 0).astype(np.int32)  # room for the appended record
    for k, w in (("d_obs_order", np.int32), ("d_obs_level", np.int32), ("d_obs_type", np.uint8)):
        m.a[k] = np.append(m.a[k], 0).astype(w)
    for k, w in (("d_obs_px", 2), ("d_obs_f", 3), ("d_obs_grad", 2)):
        m.a[k] = np.vstack([m.a[k], np.zeros((1, w))])
    m.patch(touched, mp["pos"][touched], mp["type"][touched], mp["order"][touched], mp["obs_begin"][touched], mp["obs_count"][touched],
            obs_index=[O], obs_frame=mp["obs_frame"][O:], obs_order=mp["obs_order"][O:], obs_level=mp["obs_level"][O:],
            obs_type=mp["obs_type"][O:], obs_px=mp["obs_px"][O:], obs_f=mp["obs_f"][O:], obs_grad=mp["obs_grad"][O:])
    compare(m.reproject(cam, mp["T"], mp["cur"], mp["kf_rank"], mp), oracle_reproject_map(mp, cam), P + 1, 1e-12)
