"""Row N2 on the device, at the edges: the named cases of tests/map_mirror_cases.py -- the cases of
tests/test_map_mirror_edges_emulated.py, here with the device's LDS atomics, wave scans, division and sqrt -- under the same one
rule: integers identical to the independent walk of tests/map_walk_reference.py and to the oracle, pixels to 1e-9 px of the
oracle (the bound of tests/test_map_mirror_gpu.py) and to 1e-10 + 1e-13 |px| of the mpmath walk, outputs poisoned and guarded.
The map records and the patches go through rpg_svo_amd.map_mirror.MapMirror; the call itself is the raw C entry, because
MapMirror.reproject allocates zeroed outputs of its own and raises on an error code.  Every launch is one workgroup; a case is a
handful of launches and one read-back each.  Then the entry's argument checks, row by row.

Measured on an MI355X (largest px difference per case: to the oracle, of 1e-9 / to the mpmath walk, of 1e-10 + 1e-13 |px|):
records_8_and_9 0 / 3.4e-13, many_views 0 / 2.3e-13 (radtan 0 / 1.7e-13, atan 1.1e-13 / 2.3e-13), crowded_cell 0 / 5.7e-14,
behind_camera 0 / 8.0e-13 (radtan 0 / 7.1e-13, atan 2.3e-13 / 3.4e-13), key_limits 0 / 1.7e-13, small_cells 0 / 3.4e-13,
cell_limit 0 / 3.4e-13, exact_edges 0 / 0, close_view_ties 0 / 1.1e-13, in_frame_limit 2.3e-13 / 9.1e-13, cuts 0 / 2.3e-13,
capacities 1.1e-13 / 3.4e-13, patch_moves_first_meeting 0 / 1.7e-13; every integer output identical on every case, the point at
cos == 0.5 a trial, the argument table as stated."""
import pytest
import torch

import map_mirror_cases as mc
from map_mirror_host import patch_mirror
from rpg_svo_amd import capi
from rpg_svo_amd.map_mirror import MapMirror
from rpg_svo_amd.pyramid import _stream_ptr

pytestmark = pytest.mark.gpu
PX_TOL_ORACLE = 1e-9


def make_call(dev, cam, step, m=None):
    """-> (the call as a dict of map_mirror_cases.CALL_ORDER, fetch() -> the Outputs as the device holds them, the mirror)"""
    mp = step.mp
    if m is None:
        m = MapMirror(max(mp["pos"].shape[0], 1), max(mp["obs_frame"].shape[0], 1), dev)
    patch_mirror(m, step)
    p, n_pts, n_obs = m._pending
    m._pending = None
    g = lambda k: p[k].data_ptr() if k in p else None
    patch = capi.MapPatch(n_pts, n_obs, g("index"), g("pos"), g("type"), g("order"), g("obs_begin"), g("obs_count"), g("obs_index"), g("obs_order"),
                          capi.Features(g("obs_frame"), g("obs_level"), g("obs_type"), g("obs_px"), g("obs_f"), g("obs_grad")))
    T = torch.as_tensor(mp["T"], dtype=torch.float64, device=dev).contiguous()
    rank = torch.as_tensor(mp["kf_rank"], dtype=torch.int32, device=dev)
    cell_rank = torch.as_tensor(mp["cell_rank"], dtype=torch.int32, device=dev)
    out = mc.outputs_for(step)
    raw = {k: torch.from_numpy(r).to(dev) for k, r in out.raw.items()}
    call = dict(cam=capi.camera(cam), frames=capi.Frames(T.shape[0], 0, None, T.data_ptr()), cur_frame=int(mp["cur"]), d_kf_rank=rank.data_ptr(),
                map=m.struct(), patch=patch, grid=capi.Grid(mp["cell_size"], mp["n_cols"], mp["n_rows"], mp["n_cols"] * mp["n_rows"], cell_rank.data_ptr()),
                first_cell=step.first_cell, max_cells_with_trials=min(step.max_cells, 1 << 30), max_visits=step.max_visits, max_trials=step.max_trials,
                out=out.struct({k: t.data_ptr() for k, t in raw.items()}))

    def fetch(keep=(p, T, rank, cell_rank, m)):
        torch.cuda.synchronize()
        for k, t in raw.items():
            out.raw[k][:] = t.cpu().numpy()
        return out
    return call, fetch, m


def run_case(lib, dev, c):
    outs, m = [], None
    for s in c.steps:
        call, fetch, m = make_call(dev, c.cam, s, None if s.touched is None else m)
        assert mc.invoke(lib, call, _stream_ptr(dev)) == mc.OK, (c.name, s.label)
        outs.append(fetch())
    return outs


@pytest.mark.parametrize("name,kind", mc.CASES, ids=mc.CASE_IDS)
def test_device_edges(hip_lib, gpu_device, oracle, name, kind):
    c = mc.case(name, kind)
    d_oracle, d_walk = mc.check_case(c, run_case(hip_lib, gpu_device, c), PX_TOL_ORACLE)
    print(f"{name}-{kind}: largest px difference {d_oracle:.3g} to the oracle, {d_walk:.3g} to the mpmath walk")


def test_device_argument_table(hip_lib, gpu_device, oracle):
    mc.check_arguments(hip_lib, lambda cam, step: make_call(gpu_device, cam, step)[:2], PX_TOL_ORACLE, _stream_ptr(gpu_device))
