"""TEST INFRASTRUCTURE.  The host-emulated build of K11 (rpg_svo_amd/csrc/frame_close.hip): tests/host/emu_tu_frame_close.cpp and
emu_tu_common.cpp compiled with tests/emu_build.py's flags into build/emu/libsvo_hip_frame_close_emulated.so, and the unit's
stand-alone sanitizer program (tests/host/frame_close_asan_main.cpp) with the same flags plus AddressSanitizer and
UndefinedBehaviorSanitizer.  A builder of its own until the unit is folded into emu_build.UNITS."""
import ctypes as C
import os
import subprocess

import pytest

import emu_build
from emu_build import ROOT

UNIT_SOURCES = ("emu_tu_common.cpp", "emu_tu_frame_close.cpp")


def _build(target, sources, extra):
    from rpg_svo_amd.build import DEFAULT_DEFINES
    cxx = emu_build._cxx()
    if not os.path.exists(cxx):
        pytest.skip("no ROCm clang++ to compile the kernels for the host")
    out = os.path.join(ROOT, "build", "emu", target)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "host", f) for f in sources]
    deps = [*srcs, *emu_build._kernel_deps(), os.path.abspath(__file__), os.path.abspath(emu_build.__file__)]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.run([cxx, *emu_build._kernel_cxxflags(DEFAULT_DEFINES), *extra, *srcs, "-o", out], check=True)
    return out


def build_frame_close_emulated():
    """-> the CDLL of the emulated svo_hip_frame_close / svo_hip_frame_close_params_default, prototypes bound"""
    from rpg_svo_amd import capi
    lib = C.CDLL(_build("libsvo_hip_frame_close_emulated.so", UNIT_SOURCES, ["-shared"]))
    for name in ("svo_hip_frame_close", "svo_hip_frame_close_params_default"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = capi.PROTOTYPES[name]
    return lib


def build_frame_close_asan_program():
    """-> the path of build/emu/frame_close_asan: one executable instrumented with AddressSanitizer and
    UndefinedBehaviorSanitizer (a program of its own: nothing is loaded into Python)"""
    return _build("frame_close_asan", (*UNIT_SOURCES, "frame_close_asan_main.cpp"),
                  ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-sanitize=vptr,function", "-fno-omit-frame-pointer", "-g"])
