"""TEST INFRASTRUCTURE.  rpg_svo_amd/csrc/first_map.hip (K10) compiled for the host through tests/host/hip_emu.h, like the
units of tests/emu_build.py but as a library of its own: build/emu/libsvo_hip_first_map_emulated.so holds
tests/host/emu_tu_first_map.cpp and emu_tu_common.cpp, compiled by emu_build's compiler with emu_build's flags.  Also the
stand-alone sanitizer program of tests/host/first_map_asan_main.cpp (an executable: nothing is loaded into Python)."""
import ctypes as C
import glob
import os
import subprocess

import pytest

import emu_build

ROOT = emu_build.ROOT
UNITS = ("common", "first_map")
# the compile line of emu_build.build_emulated
CXXFLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-fno-math-errno", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-pass-failed",
            "-Wno-unused-function", "-Wno-unused-variable"]


def _includes():
    return ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rpg_svo_amd", "csrc"), "-I", os.path.join(ROOT, "tests", "host")]


def _sources(extra=()):
    host = os.path.join(ROOT, "tests", "host")
    return [os.path.join(host, f"emu_tu_{u}.cpp") for u in UNITS] + [os.path.join(host, e) for e in extra]


def _stale(target, sources):
    csrc = os.path.join(ROOT, "rpg_svo_amd", "csrc")
    deps = list(sources) + glob.glob(os.path.join(csrc, "*.h")) + [os.path.join(csrc, "first_map.hip"), os.path.join(ROOT, "include", "svo_hip.h"),
                                                                  os.path.join(ROOT, "tests", "host", "hip_emu.h"), os.path.abspath(__file__)]
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(d) for d in deps)


def _cxx_or_skip():
    cxx = emu_build._cxx()
    if not os.path.exists(cxx):
        pytest.skip("no ROCm clang++ to compile the kernels for the host")
    return cxx


def build_first_map_emulated():
    """-> the library as a ctypes handle, with both entries' prototypes bound as rpg_svo_amd.capi declares them"""
    from rpg_svo_amd import capi
    from rpg_svo_amd.build import DEFAULT_DEFINES
    cxx = _cxx_or_skip()
    san = emu_build.sanitizer()
    lib_path = os.path.join(ROOT, "build", "emu", f"libsvo_hip_first_map_emulated{'_' + san if san else ''}.so")
    os.makedirs(os.path.dirname(lib_path), exist_ok=True)
    srcs = _sources()
    if _stale(lib_path, srcs):
        subprocess.run([cxx, *CXXFLAGS, *emu_build._sanitizer_flags(san), *[f"-D{d}" for d in DEFAULT_DEFINES], *_includes(), "-shared",
                        *srcs, "-o", lib_path], check=True)
    lib = C.CDLL(lib_path)
    for name in ("svo_hip_first_map", "svo_hip_initialize_seeds"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = capi.PROTOTYPES[name]
    return lib


def build_first_map_asan_program():
    """-> the path of build/emu/first_map_asan: the emulated units and tests/host/first_map_asan_main.cpp, one executable
    instrumented with AddressSanitizer and UndefinedBehaviorSanitizer"""
    cxx = _cxx_or_skip()
    exe = os.path.join(ROOT, "build", "emu", "first_map_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    srcs = _sources(("first_map_asan_main.cpp",))
    if _stale(exe, srcs):
        subprocess.run([cxx, *CXXFLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-sanitize=vptr,function",
                        "-fno-omit-frame-pointer", "-g", *_includes(), *srcs, "-o", exe], check=True)
    return exe
