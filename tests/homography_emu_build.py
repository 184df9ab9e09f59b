"""TEST INFRASTRUCTURE.  The host-emulated build of the homography unit: rpg_svo_amd/csrc/homography_init.hip compiled as plain
C++ through tests/host/hip_emu.h (tests/host/emu_tu_homography_init.cpp) and linked with the common unit of the emulated
library into build/emu/libsvo_hip_emulated_homography[_<sanitizer>].so.  Same compiler and flags as tests/emu_build.py
and tests/klt_emu_build.py, whose unit lists are fixed; SVO_EMU_SANITIZE is honoured the same way."""
import ctypes as C
import glob
import os
import subprocess

import pytest

from emu_build import ROOT, llvm_bin, sanitizer

UNITS = ("common", "homography_init")


def build_emulated_homography():
    san = sanitizer()
    san_flags = [f"-fsanitize={san}", "-shared-libsan", "-fno-omit-frame-pointer", "-g"] if san else []
    if san == "undefined":
        san_flags += ["-fsanitize=float-cast-overflow", "-fno-sanitize=vptr,function"]
    tag = "_homography" + ("_" + san if san else "")
    lib_path = os.path.join(ROOT, "build", "emu", f"libsvo_hip_emulated{tag}.so")
    objdir = os.path.join(ROOT, "build", "emu", f"obj{tag}")
    os.makedirs(objdir, exist_ok=True)
    csrc = os.path.join(ROOT, "rpg_svo_amd", "csrc")
    cxx = os.path.join(llvm_bin(), "clang++")
    if not os.path.exists(cxx):
        pytest.skip("no ROCm clang++ to compile the kernels for the host")
    deps = glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(csrc, "*.hip")) + \
        [os.path.join(ROOT, "include", "svo_hip.h"), os.path.join(ROOT, "tests", "host", "hip_emu.h")]
    newest = max(os.path.getmtime(d) for d in deps)
    stamp, flags_now = os.path.join(objdir, "flags.txt"), " ".join([*san_flags, "-O1"])
    if not os.path.exists(stamp) or open(stamp).read() != flags_now:
        for o in glob.glob(os.path.join(objdir, "*.o")):
            os.remove(o)
        open(stamp, "w").write(flags_now)
    objs, todo = [], []
    for u in UNITS:
        src = os.path.join(ROOT, "tests", "host", f"emu_tu_{u}.cpp")
        obj = os.path.join(objdir, f"{u}.o")
        objs.append(obj)
        if not os.path.exists(obj) or os.path.getmtime(obj) < max(newest, os.path.getmtime(src)):
            todo.append([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fno-math-errno", "-fPIC", "-c", "-Wall", "-Wno-unknown-pragmas",
                         "-Wno-pass-failed", "-Wno-unused-function", "-Wno-unused-variable", *san_flags,
                         "-I", os.path.join(ROOT, "include"), "-I", csrc, "-I", os.path.join(ROOT, "tests", "host"), src, "-o", obj])
    if todo:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=len(todo)) as ex:
            list(ex.map(lambda cmd: subprocess.run(cmd, check=True), todo))
    if not os.path.exists(lib_path) or any(os.path.getmtime(o) > os.path.getmtime(lib_path) for o in objs):
        subprocess.run([cxx, "-shared", *san_flags, "-o", lib_path, *objs], check=True)
    return C.CDLL(lib_path)
