"""TEST INFRASTRUCTURE: svo_hip_keyframe_insert's host-emulated backend.  tests/emu_build.py's library has a fixed unit list, so
K12 runs as a PROGRAM: emu_tu_common.cpp, emu_tu_keyframe_insert.cpp and keyframe_insert_main.cpp built by
emu_build.build_program (plain for the bit comparison, with AddressSanitizer and UndefinedBehaviorSanitizer for
tests/test_keyframe_insert_sanitized.py).  This module writes the case files, starts the program and reads the results back.
The program takes the emulator's schedule as an argument and sets it itself; every array lies between guard bands there and
the outputs start poisoned.  Nothing is loaded into Python."""
import os
import subprocess

import numpy as np

import keyframe_insert_checker as chk
from emu_build import build_program, run_program

SOURCES = ("emu_tu_common.cpp", "emu_tu_keyframe_insert.cpp", "keyframe_insert_main.cpp")
SCHEDULES = ("inorder", "reverse", "waves")
MAGIC = 0x4b313249


def program(sanitize=False):
    return build_program("keyframe_insert_asan" if sanitize else "keyframe_insert_prog", SOURCES, sanitize=sanitize)


def write_case(b, path):
    K, F, P, R = b.dims
    with open(path, "wb") as fh:
        fh.write(np.array([MAGIC, b.B, b.n_stride, K, F, P, R, b.cam.width, b.cam.height, len(b.inputs)], np.int32).tobytes())
        for k, (shape, dt) in chk.state_shapes(b.B, *b.dims).items():
            a = np.ascontiguousarray(b.state[k])
            assert a.shape == shape and a.dtype == dt, k
            fh.write(a.tobytes())
        for inp in b.inputs:
            for k in chk.INPUTS:
                fh.write(np.ascontiguousarray(inp[k]).tobytes())


def read_result(b, path):
    """-> per call (return code, state, outputs)"""
    raw = open(path, "rb").read()
    at, calls = 0, []

    def take(shape, dt):
        nonlocal at
        n = int(np.prod(shape)) * np.dtype(dt).itemsize
        a = np.frombuffer(raw[at:at + n], dt).reshape(shape).copy()
        at += n
        return a

    for _ in b.inputs:
        rc = int(take((1,), np.int32)[0])
        state = {k: take(shape, dt) for k, (shape, dt) in chk.state_shapes(b.B, *b.dims).items()}
        out = {k: take((b.B,), np.int32) for k in chk.OUTPUTS}
        calls.append((rc, state, out))
    assert at == len(raw), (at, len(raw))
    return calls


def run(batches, schedule, tmp_dir, sanitize=False):
    """the batches (name -> batch) through one process of the program -> name -> per call (return code, state, outputs)"""
    exe = program(sanitize)
    args = []
    for name, b in batches.items():
        case, result = os.path.join(tmp_dir, f"{name}.case"), os.path.join(tmp_dir, f"{name}.{schedule}.result")
        write_case(b, case)
        args += [case, result]
    if sanitize:
        run_program(exe, "run", schedule, *args)
    else:
        r = subprocess.run([exe, "run", schedule, *args], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-2000:])
    return {name: read_result(b, args[2 * i + 1]) for i, (name, b) in enumerate(batches.items())}


def compare(got, b, what=""):
    """every state array and every output of every call: the checker's bytes"""
    from host_buffers import same_bits
    assert len(got) == len(b.expect)
    for c, ((rc, state, out), (want_state, want_out)) in enumerate(zip(got, b.expect)):
        assert rc == 0, (what, c, rc)
        for k in chk.OUTPUTS:
            assert same_bits(out[k], want_out[k]), (what, c, k, out[k].tolist(), want_out[k].tolist())
        for k in chk.STATE:
            if not same_bits(state[k], want_state[k]):
                g, w = state[k].reshape(b.B, -1), np.asarray(want_state[k]).reshape(b.B, -1)
                where = [(s, int(np.flatnonzero(g[s].view(np.uint8) != w[s].view(np.uint8))[0])) for s in range(b.B) if not same_bits(g[s], w[s])]
                raise AssertionError((what, c, k, "first differing (sequence, byte)", where[:4]))
