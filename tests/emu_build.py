"""TEST INFRASTRUCTURE.  The host-emulated build of the C-ABI library: the .hip translation units of rpg_svo_amd/csrc compiled by
ROCm's clang++ as plain C++ through tests/host/hip_emu.h (work-items as fibers, barriers, LDS, cross-lane rendezvous) and
linked into build/emu/libsvo_hip_emulated[_<defines>][_<sanitizer>].so: ONE library with every kernel family, the entry points of
libsvo_hip.so's kernel files on host memory; no timing.  Also THE recipe of a stand-alone sanitizer program (build_program,
run_program): emulated units and a main of their own, compiled with the same flags."""
import ctypes as C
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ("common", "pyramid", "map_mirror", "matcher", "feature_align", "depth_filter", "sparse_align", "sparse_align_wave",
         "pose_optimizer_wave", "pose_optimizer", "point_optimizer", "fast_detect", "klt_track", "homography_init", "first_map",
         "frame_close")


# Compile-time variants of the library the emulated parity tests run on besides the default build (round 4 queued ten of
# them for timing; round 5 measured them on the GPU, the winners became the only code and the losers were deleted:
# profiles/r05a_queue_drain.txt).  Tests take their build from this list: a new opt-in flag is one more tuple here.
# Round 6: ("ALIGN_WAVE_MAX_M_VALUE=0",) -- no batch is small enough for the wave-per-trial alignment, so the depth filter's
# small test batches take the lane-per-trial kernel WITH the seed_finish epilogue (csrc/seed_finish.h), the path of replay
# batches beyond 8192 seeds.
# ("SIA_F64_PARTIALS",) -- the reference-width build of K1 (csrc/sparse_align.hip: per-pixel products, patch sums and SE3::exp
# in f64, the scalar pixel loop instead of the packed one), the library behind the benchmark's `roofline_f64_build` figure.
# Only sparse_align.hip reads the define: the K1 tests (tests/k1_emulated.py's K1_BUILDS: test_sparse_align_emulated.py,
# test_k1_level_arith_emulated.py, test_emulated_shapes.py) run builds 0 and 2 on the cases tests/k1_cases.py gives them.
BUILDS = [(), ("ALIGN_WAVE_MAX_M_VALUE=0",), ("SIA_F64_PARTIALS",)]
BUILD_IDS = ["default", "lane_kernel_with_finish", "reference_width"]


def sanitizer():
    """SVO_EMU_SANITIZE=address|thread: the emulated library instrumented by that sanitizer (the process must have the
    runtime preloaded: scripts/emu_sanitize.sh)."""
    return os.environ.get("SVO_EMU_SANITIZE", "")


def llvm_bin():
    """ROCm's LLVM tools: clang++, its sanitizer runtimes, and the llvm-symbolizer their reports need for source lines"""
    return os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")


def _cxx():
    return os.path.join(llvm_bin(), "clang++")


def _sanitizer_flags(san):
    """compile and link flags of a build instrumented by sanitizer `san` ("": none)"""
    if not san:
        return []
    flags = [f"-fsanitize={san}", "-shared-libsan", "-fno-omit-frame-pointer", "-g"]
    if san == "undefined":
        # + float-cast-overflow (a float -> int conversion out of range: the kernels guard theirs to reproduce cvttss2si).
        # float-divide-by-zero stays off: IEEE defines it and the kernels rely on it where the reference does (1 / tau2 with
        # tau2 = 0, the inverse of a singular H, chi2 / n_meas with nothing tracked: six sites, all the reference's own)
        flags += ["-fsanitize=float-cast-overflow", "-fno-sanitize=vptr,function"]
    return flags


def sanitizer_runtime(kind):
    name = {"address": "asan", "thread": "tsan", "undefined": "ubsan_standalone"}[kind]
    out = subprocess.run([_cxx(), f"-print-file-name=libclang_rt.{name}-x86_64.so"], capture_output=True, text=True).stdout.strip()
    return out if os.path.isabs(out) and os.path.exists(out) else None


def build_race_probe():
    """tests/host/emu_race_probe.cpp (a kernel with and without the barrier it needs) with the sanitizer of SVO_EMU_SANITIZE."""
    san = sanitizer()
    lib_path = os.path.join(ROOT, "build", "emu", f"libemu_race_probe_{san or 'plain'}.so")
    src = os.path.join(ROOT, "tests", "host", "emu_race_probe.cpp")
    hdr = os.path.join(ROOT, "tests", "host", "hip_emu.h")
    os.makedirs(os.path.dirname(lib_path), exist_ok=True)
    if not os.path.exists(lib_path) or os.path.getmtime(lib_path) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run([_cxx(), "-std=c++17", "-O1", "-fPIC", "-shared", *_sanitizer_flags(san), "-I", os.path.join(ROOT, "tests", "host"),
                        src, "-o", lib_path], check=True)
    lib = C.CDLL(lib_path)
    lib.probe_neighbour_sum.restype = C.c_int
    lib.probe_neighbour_sum.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    return lib


def _kernel_cxxflags(defines):
    """THE compile flags of the kernel files for the host: the objects of build_emulated and the stand-alone sanitizer program"""
    return ["-std=c++17", "-O1", "-ffp-contract=off", "-fno-math-errno", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-pass-failed",
            "-Wno-unused-function", "-Wno-unused-variable", *[f"-D{d}" for d in defines], "-I", os.path.join(ROOT, "include"),
            "-I", os.path.join(ROOT, "rpg_svo_amd", "csrc"), "-I", os.path.join(ROOT, "tests", "host")]


def _kernel_deps():
    """what every emulated translation unit is rebuilt after, besides its own emu_tu_*.cpp"""
    csrc = os.path.join(ROOT, "rpg_svo_amd", "csrc")
    return glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(csrc, "*.hip")) + \
        [os.path.join(ROOT, "include", "svo_hip.h"), os.path.join(ROOT, "tests", "host", "hip_emu.h")]


def build_emulated(defines=(), bind=()):
    """-> a fresh CDLL of the emulated library built with `defines`; the entries named in `bind` get capi.PROTOTYPES' prototypes"""
    # SVO_EMU_EXTRA_DEFINES="A B": added to every emulated build of the run (e.g. the whole round-5 queue on the default tests)
    from rpg_svo_amd.build import DEFAULT_DEFINES   # (the default library's own flags: the emulated default build has them too)
    defines = tuple(dict.fromkeys(tuple(DEFAULT_DEFINES) + tuple(defines) + tuple(os.environ.get("SVO_EMU_EXTRA_DEFINES", "").split())))
    tag = "".join("_" + d.replace("=", "-") for d in defines)
    if len(tag) > 80:
        import hashlib
        tag = "_set" + hashlib.sha1(tag.encode()).hexdigest()[:10]
    san = sanitizer()
    san_flags = _sanitizer_flags(san)
    if san:
        tag += "_" + san
    lib_path = os.path.join(ROOT, "build", "emu", f"libsvo_hip_emulated{tag}.so")
    objdir = os.path.join(ROOT, "build", "emu", f"obj{tag}")
    os.makedirs(objdir, exist_ok=True)
    cxx = _cxx()
    if not os.path.exists(cxx):
        pytest.skip("no ROCm clang++ to compile the kernels for the host")
    newest = max(os.path.getmtime(d) for d in _kernel_deps())
    # (a change of flags rebuilds too: the object directory remembers what it was compiled with)
    stamp, flags_now = os.path.join(objdir, "flags.txt"), " ".join([*san_flags, *defines, "-O1"])
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
            todo.append([cxx, *_kernel_cxxflags(defines), *san_flags, "-c", src, "-o", obj])
    if todo:  # the translation units in parallel: a cold build of one variant set takes about as long as its slowest unit
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(8, len(todo))) as ex:
            list(ex.map(lambda cmd: subprocess.run(cmd, check=True), todo))
    if not os.path.exists(lib_path) or any(os.path.getmtime(o) > os.path.getmtime(lib_path) for o in objs):
        subprocess.run([cxx, "-shared", *san_flags, "-o", lib_path, *objs], check=True)
    lib = C.CDLL(lib_path)   # (a CDLL object of the caller's own: argtypes belong to the object, and other callers pass raw pointers)
    if bind:
        from rpg_svo_amd import capi
        for name in bind:
            getattr(lib, name).restype, getattr(lib, name).argtypes = capi.PROTOTYPES[name]
    return lib


def build_program(name, sources, sanitize=True, extra_checks=(), deps=()):
    """-> the path of build/emu/<name>: the files `sources` of tests/host (emulated units and a *_main.cpp) compiled with the
    library's flags into one executable, instrumented with AddressSanitizer and UndefinedBehaviorSanitizer unless `sanitize` is
    False (a program of its own: nothing is loaded into Python).  `extra_checks`: further -fsanitize= groups; `deps`: what it is
    rebuilt after besides its sources, the kernel files and this file (names in tests/host, or paths)."""
    from rpg_svo_amd.build import DEFAULT_DEFINES
    cxx = _cxx()
    if not os.path.exists(cxx):
        pytest.skip("no ROCm clang++ to compile the kernels for the host")
    exe = os.path.join(ROOT, "build", "emu", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    host = os.path.join(ROOT, "tests", "host")
    srcs = [os.path.join(host, f) for f in sources]
    after = [*srcs, *_kernel_deps(), os.path.abspath(__file__), *[os.path.join(host, d) for d in deps]]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in after):
        san = ["-fsanitize=address,undefined", *[f"-fsanitize={c}" for c in extra_checks], "-fno-sanitize-recover=undefined",
               "-fno-sanitize=vptr,function", "-fno-omit-frame-pointer", "-g"] if sanitize else []
        subprocess.run([cxx, *_kernel_cxxflags(DEFAULT_DEFINES), *san, *srcs, "-o", exe], check=True)
    return exe


def run_program(exe, *args):
    """runs a program of build_program: no sanitizer report, exit code 0, last line "ok" -> the finished process"""
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600, env={"ASAN_OPTIONS": "detect_leaks=0"})
    print(r.stdout)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-4000:], r.stderr[-2000:])
    return r
