"""The checker of K12 (tests/keyframe_insert_checker.py) against the reference itself (CPU; skipped where the reference checkout
is absent).  tests/host/ref_keyframe_insert.cpp is compiled into build/ref_keyframe_insert/ against oracle/shim together with
the reference's frame.cpp, point.cpp, config.cpp, feature_detection.cpp and map.cpp, where they lie.  From the flattened map of
a sequence it builds real Frame / Feature / Point objects and a Map with its candidate list, makes the calls of
frame_handler_mono.cpp:196-200, 224-232 (setKeyframe() replaced by the given key points, the depth-filter calls left out) and
flattens the lists back.  For every acting sequence of every well-formed case, after every call, every field the reference
has must equal the checker's: kf_list; table length, key points and rows (px, f, level, point) of every keyframe of the list;
type and n_obs of every point; the records (keyframe, row, level, px, f) of every living point, in list order.

What the reference has no notion of is defined by the header and pinned by the checker alone: the bytes beyond a list's end,
the freed slot, the choice of the storage slot, the capacities (sequences whose status is not 0 are not run: the reference
has no capacity), and the cases whose indices cannot index (`well_formed` False: bad_indices, bad_kf_remove, bad_kf_list) --
the reference would follow a dangling pointer there.

Measured: 0 differences over the 34 well-formed batches (89 acting sequences that fit their capacities)."""
import ctypes as C
import os

import numpy as np
import pytest

import keyframe_insert_cases as cases
import keyframe_insert_checker as chk
from host_buffers import same_bits
from oracle.pytrack import build_ref_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_UNITS = ("frame", "point", "config", "feature_detection", "map")
PER_SEQUENCE = ("kf_list", "kf_n_fts", "kf_key_pts", "ftr_px", "ftr_f", "ftr_level", "ftr_point", "pt_pos", "pt_type", "pt_order", "pt_n_obs",
                "obs_kf", "obs_row", "obs_level", "obs_px", "obs_f")


@pytest.fixture(scope="module")
def ref():
    lib_path = build_ref_harness(os.path.join(ROOT, "tests", "host", "ref_keyframe_insert.cpp"), REF_UNITS, "ref_keyframe_insert")
    if lib_path is None:
        pytest.skip("no reference checkout to compile frame.cpp / point.cpp / map.cpp from")
    lib = C.CDLL(lib_path)
    lib.ref_keyframe_insert.restype = C.c_int
    lib.ref_keyframe_insert.argtypes = [C.c_int] * 6 + [C.c_void_p] * 17 + [C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_int]
    return lib


def sequence_of(state, b, dims):
    """the arrays of sequence b as the harness takes them: its own copy, frames named by slot"""
    K, F, P, R = dims
    B = state["kf_list"].shape[0]
    s = {k: np.ascontiguousarray(np.asarray(state[k]).reshape(B, -1)[b]).copy() for k in PER_SEQUENCE}
    s["n_kf"] = np.array([state["n_kf"][b]], np.int32)
    live = (np.arange(R)[None, :] < state["pt_n_obs"][b][:, None]) & (state["pt_type"][b] != 0)[:, None]
    s["obs_kf"] = np.where(live.ravel(), s["obs_kf"] - b * K, 0).astype(np.int32)
    return s


def lists_of(s, dims):
    """what the reference has: the lists, without the bytes beyond their ends"""
    K, F, P, R = dims
    n_kf = int(s["n_kf"][0])
    view = {"kf_list": [int(v) for v in s["kf_list"][:n_kf]]}
    for slot in view["kf_list"]:
        k = int(s["kf_n_fts"][slot])
        rows = slice(slot * F, slot * F + k)
        view[f"kf{slot}"] = (k, s["kf_key_pts"][5 * slot:5 * slot + 5].tolist(), s["ftr_px"].reshape(-1, 2)[rows].tobytes(),
                             s["ftr_f"].reshape(-1, 3)[rows].tobytes(), s["ftr_level"][rows].tolist(), s["ftr_point"][rows].tolist())
    for p in range(P):
        t, k = int(s["pt_type"][p]), int(s["pt_n_obs"][p])
        rec = slice(p * R, p * R + (k if t else 0))
        view[f"pt{p}"] = (t, k if t else 0, s["obs_kf"][rec].tolist(), s["obs_row"][rec].tolist(), s["obs_level"][rec].tolist(),
                          s["obs_px"].reshape(-1, 2)[rec].tobytes(), s["obs_f"].reshape(-1, 3)[rec].tobytes())
    return view


@pytest.mark.parametrize("name", [n for n in cases.NAMES if cases.batches()[n].well_formed])
def test_checker_has_the_references_lists(ref, name):
    b = cases.batches()[name]
    K, F, P, R = b.dims
    cur, compared = b.state, 0
    for inp, (want_state, want_out) in zip(b.inputs, b.expect):
        for s in range(b.B):
            if inp["result"][s] != cases.IS_KF or want_out["status"][s] != 0:
                continue
            seq = sequence_of(cur, s, b.dims)
            n = min(max(int(inp["n"][s]), 0), b.n_stride)
            # the point behind a row, as the header states it: has_point, a living point, the first row of a point keeps it
            point, seen = np.full(max(n, 1), -1, np.int32), set()
            for j in range(n):
                p = int(inp["ftr_point"][s, j])
                if inp["has_point"][s, j] and 0 <= p < P and cur["pt_type"][s, p] != 0 and p not in seen:
                    point[j] = p
                    seen.add(p)
            px, f, level = (np.ascontiguousarray(inp[k][s]) for k in ("px", "f", "level"))
            key_pts = np.ascontiguousarray(inp["key_pts"][s], np.int32)
            rm = int(inp["kf_remove"][s])
            rc = ref.ref_keyframe_insert(b.cam.width, b.cam.height, K, F, P, R, *[seq[k].ctypes.data for k in ("n_kf",) + PER_SEQUENCE], n,
                                         px.ctypes.data, f.ctypes.data, level.ctypes.data, point.ctypes.data, key_pts.ctypes.data,
                                         rm if 0 <= rm < int(cur["n_kf"][s]) else -1, int(want_out["kf_new_slot"][s]))
            assert rc == 0, (name, s, rc)
            got, want = lists_of(seq, b.dims), lists_of(sequence_of(want_state, s, b.dims), b.dims)
            assert got.keys() == want.keys() and got["kf_list"] == want["kf_list"], (name, s, got["kf_list"], want["kf_list"])
            for k in want:
                assert got[k] == want[k], (name, s, k, got[k][:5], want[k][:5])
            types = seq["pt_type"]
            assert int(((cur["pt_type"][s] == 1) & (types == 2)).sum()) <= want_out["n_promoted"][s]    # (some leave with their keyframe)
            assert int(((cur["pt_type"][s] != 0) & (types == 0)).sum()) == want_out["n_points_deleted"][s]
            compared += 1
        cur = want_state
    print(f"{name}: {compared} sequences compared with the reference")
    assert compared or name in ("bad_kf_list",)
