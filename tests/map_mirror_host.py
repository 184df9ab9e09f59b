"""TEST INFRASTRUCTURE (numpy and ctypes only).  svo_hip_reproject_map on host memory, for the host-emulated library: `HostMirror`
keeps the records of svo_hip_map in host arrays (what rpg_svo_amd.map_mirror.MapMirror keeps in device tensors), `upload` fills one
from a plain-array map, `compare` is the rule of tests/test_map_mirror_emulated.py against the oracle; `make_call` / `run_case` are
the emulated backend of tests/map_mirror_cases.py (poisoned, guarded outputs; the call as a dict the argument table can spoil)."""
import numpy as np

import map_mirror_cases as mc
from host_buffers import ptr
from rpg_svo_amd import capi


class HostMirror:
    """the records of svo_hip_map in host arrays (what rpg_svo_amd.map_mirror.MapMirror keeps in device tensors)"""

    def __init__(self, lib, P, O):
        self.lib = lib
        self.n_points = self.n_obs = 0
        self.a = dict(d_pos=np.zeros((P, 3)), d_type=np.zeros(P, np.int32), d_order=np.zeros(P, np.int32), d_obs_begin=np.zeros(P, np.int32),
                      d_obs_count=np.zeros(P, np.int32), d_obs_frame=np.zeros(O, np.int32), d_obs_order=np.zeros(O, np.int32),
                      d_obs_level=np.zeros(O, np.int32), d_obs_type=np.zeros(O, np.uint8), d_obs_px=np.zeros((O, 2)),
                      d_obs_f=np.zeros((O, 3)), d_obs_grad=np.zeros((O, 2)))
        self.pending = None

    def patch(self, index, pos, type, order, obs_begin, obs_count, obs_index=None, obs_frame=None, obs_order=None, obs_level=None,
              obs_type=None, obs_px=None, obs_f=None, obs_grad=None):
        c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
        index = c(index, np.int32)
        p = dict(index=index, pos=c(pos, np.float64).reshape(-1, 3), type=c(type, np.int32), order=c(order, np.int32),
                 obs_begin=c(obs_begin, np.int32), obs_count=c(obs_count, np.int32))
        if index.size:
            self.n_points = max(self.n_points, int(index.max()) + 1)
        n_obs = 0 if obs_index is None else len(obs_index)
        if n_obs:
            oi = c(obs_index, np.int32)
            self.n_obs = max(self.n_obs, int(oi.max()) + 1)
            p.update(obs_index=oi, obs_frame=c(obs_frame, np.int32), obs_order=c(obs_order, np.int32), obs_level=c(obs_level, np.int32),
                     obs_type=c(obs_type, np.uint8), obs_px=c(obs_px, np.float64).reshape(-1, 2), obs_f=c(obs_f, np.float64).reshape(-1, 3),
                     obs_grad=c(obs_grad, np.float64).reshape(-1, 2))
        self.pending = (p, int(index.size), n_obs)

    def call(self, cam, T, cur, kf_rank, mp, first_cell, max_cells_with_trials, max_visits, max_trials, out_struct):
        """-> the call as a dict of tests/map_mirror_cases.py (CALL_ORDER) and what must outlive it"""
        T = np.ascontiguousarray(T, np.float64)
        kf_rank = np.ascontiguousarray(kf_rank, np.int32)
        cell_rank = np.ascontiguousarray(mp["cell_rank"], np.int32)
        patch, p = None, None
        if self.pending is not None:
            p, n_pts, n_obs = self.pending
            self.pending = None
            g = lambda k: ptr(p.get(k))
            patch = capi.MapPatch(n_pts, n_obs, g("index"), g("pos"), g("type"), g("order"), g("obs_begin"), g("obs_count"), g("obs_index"),
                                  g("obs_order"), capi.Features(g("obs_frame"), g("obs_level"), g("obs_type"), g("obs_px"), g("obs_f"), g("obs_grad")))
        call = dict(cam=capi.camera(cam), frames=capi.Frames(T.shape[0], 0, None, T.ctypes.data), cur_frame=int(cur), d_kf_rank=kf_rank.ctypes.data,
                    map=capi.Map(self.n_points, self.n_obs, *[self.a[n].ctypes.data for n, _ in capi.Map._fields_[2:]]), patch=patch,
                    grid=capi.Grid(mp["cell_size"], mp["n_cols"], mp["n_rows"], mp["n_cols"] * mp["n_rows"], cell_rank.ctypes.data),
                    first_cell=int(first_cell), max_cells_with_trials=int(min(max_cells_with_trials, 1 << 30)), max_visits=int(max_visits),
                    max_trials=int(max_trials), out=out_struct)
        return call, (T, kf_rank, cell_rank, p, self.a)

    def reproject(self, cam, T, cur, kf_rank, mp, first_cell=0, max_cells_with_trials=1 << 30, max_visits=4096, max_trials=4096):
        n_frames = T.shape[0]
        zi = lambda n: np.zeros(max(n, 1), np.int32)
        zd = lambda n, k: np.zeros((max(n, 1), k))
        P = max(self.n_points, 1)
        out = dict(d_header=zi(capi.REPROJ_HEADER), d_point_cell=zi(P), d_point_px=zd(P, 2), d_kf_count=zi(n_frames), d_visit_point=zi(max_visits),
                   d_visit_cell=zi(max_visits), d_visit_trial=zi(max_visits), d_trial_cur=zi(max_trials), d_trial_pos=zd(max_trials, 3),
                   d_trial_obs_begin=zi(max_trials), d_trial_obs_end=zi(max_trials), d_trial_cell=zi(max_trials), d_trial_px=zd(max_trials, 2))
        rs = capi.Reprojection(*[out[n].ctypes.data for n, _ in capi.Reprojection._fields_])
        call, keep = self.call(cam, T, cur, kf_rank, mp, first_cell, max_cells_with_trials, max_visits, max_trials, rs)
        rc = mc.invoke(self.lib, call)
        assert rc == 0, rc
        return out


def upload(lib, mp, capacity=None):
    P, O = mp["pos"].shape[0], mp["obs_frame"].shape[0]
    m = HostMirror(lib, capacity or max(P, 1), max(O, 1))
    m.patch(np.arange(P), mp["pos"], mp["type"], mp["order"], mp["obs_begin"], mp["obs_count"], obs_index=np.arange(O),
            obs_frame=mp["obs_frame"], obs_order=mp["obs_order"], obs_level=mp["obs_level"], obs_type=mp["obs_type"],
            obs_px=mp["obs_px"], obs_f=mp["obs_f"], obs_grad=mp["obs_grad"])
    return m


def compare(r, o, P, px_tol):
    st, E, V, M, end = [int(x) for x in r["d_header"][:5]]
    assert st == 0 and (E, V, M, end) == tuple(int(x) for x in o["header"][1:5])
    assert np.array_equal(r["d_point_cell"][:P], o["point_cell"])
    assert np.array_equal(r["d_kf_count"], o["kf_count"])
    seen = o["point_cell"] >= -1
    dpx = np.abs(r["d_point_px"][:P][seen] - o["point_px"][seen])
    assert dpx.size == 0 or dpx.max() <= px_tol, dpx.max()
    for a, b in (("d_visit_point", "visit_point"), ("d_visit_cell", "visit_cell"), ("d_visit_trial", "visit_trial")):
        assert np.array_equal(r[a][:V], o[b]), a
    assert np.array_equal(r["d_trial_obs_begin"][:M], o["trial_obs"])
    assert np.array_equal(r["d_trial_obs_end"][:M], o["trial_obs"] + 1)
    assert np.array_equal(r["d_trial_cell"][:M], o["trial_cell"])
    assert np.array_equal(r["d_trial_pos"][:M], o["trial_pos"])
    assert M == 0 or np.abs(r["d_trial_px"][:M] - o["trial_px"]).max() <= px_tol
    return V, M


# ---- the emulated backend of tests/map_mirror_cases.py -------------------------------------------------------------------------
def patch_mirror(m, step):
    """queues the step's patch on a HostMirror or a MapMirror (the same signature)"""
    idx, cols, oidx, ocols = mc.patch_of(step)
    m.patch(idx, cols["pos"], cols["type"], cols["order"], cols["obs_begin"], cols["obs_count"], obs_index=oidx, **ocols)


def make_call(lib, cam, step, m=None):
    """-> (the call, fetch() -> the Outputs as the call left them, the mirror)"""
    mp = step.mp
    if m is None:
        m = HostMirror(lib, max(mp["pos"].shape[0], 1), max(mp["obs_frame"].shape[0], 1))
    patch_mirror(m, step)
    out = mc.outputs_for(step)
    call, keep = m.call(cam, mp["T"], mp["cur"], mp["kf_rank"], mp, step.first_cell, step.max_cells, step.max_visits, step.max_trials,
                        out.struct({k: r.ctypes.data for k, r in out.raw.items()}))
    return call, (lambda keep=keep: out), m


def run_case(lib, c):
    outs, m = [], None
    for s in c.steps:
        call, fetch, m = make_call(lib, c.cam, s, None if s.touched is None else m)
        assert mc.invoke(lib, call) == mc.OK, (c.name, s.label)
        outs.append(fetch())
    return outs
