"""K1 at the reference's width on the GPU: rpg_svo_amd/lib/variants/libsvo_hip_SIA_F64_PARTIALS.so -- the build of
csrc/sparse_align.hip with the per-pixel products, the patch sums and SE3::exp in f64, the scalar pixel loop and three waves
per SIMD, the library behind the benchmark's `roofline_f64_build` figure -- against the oracle, under the device profiles of
tests/k1_cases.py: the bounds the default library holds in tests/test_sparse_align_gpu.py and tests/test_full_size_gpu.py.

rpg_svo_amd.capi binds one library per process, so ONE child process (tests/k1_width_child.py, started fresh with
SVO_HIP_LIB set) runs the variant pairs of tests/k1_cases.py's table on the variant and leaves its answers in a file; the tests
here build the same cases, run the oracle (and, where noted, the default library in this process) and apply that module's rule.  A missing variant,
a child that exits non-zero or runs into its time limit FAILS the fixture, and with it every test of the module, before any of
them starts something on the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import k1_cases as k1
import k1_device
import k1_width_child
from rpg_svo_amd import se3

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = os.path.join(ROOT, "rpg_svo_amd", "lib", "variants", "libsvo_hip_SIA_F64_PARTIALS.so")

_child = {}   # "arrays" or "failure": the child runs ONCE per session, whatever pytest does with the fixture


def _run_child(out):
    if not os.path.exists(VARIANT):
        return f"{VARIANT} is missing: build() compiles it"
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "k1_width_child.py"), out],
                           env=dict(os.environ, SVO_HIP_LIB=VARIANT), timeout=300, capture_output=True, text=True)
    except subprocess.TimeoutExpired as e:
        return f"the child on the reference-width library did not end within {e.timeout} s"
    print(r.stdout[-2000:])
    if r.returncode != 0:
        return f"the child on the reference-width library ended with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    z = np.load(out)
    _child["arrays"] = {k: z[k] for k in z.files}
    return None


class Variant:
    """the child's answers as a backend: run(case, schedule, kernel) -> K1Answer, kernel "auto", "workgroup" or "again" (the
    second run of k1_cases.VAR_TWICE)"""

    def __init__(self, arrays):
        self.arrays = arrays

    def run(self, case, schedule, kernel="auto"):
        return k1.K1Answer(**{f: self.arrays[k1_width_child.key(case.name, schedule, kernel) + f] for f in k1.FIELDS})


@pytest.fixture(scope="module")
def variant(gpu_device, tmp_path_factory):
    """the child's answers; fails (never skips) without them"""
    if not _child:
        _child["failure"] = _run_child(str(tmp_path_factory.mktemp("k1_width") / "variant.npz"))
    if _child["failure"]:
        pytest.fail(_child["failure"])
    assert str(_child["arrays"]["lib_path"]) == VARIANT
    return Variant(_child["arrays"])


_default = {}


def default_of(name):
    """the default library (this process's) on a case"""
    if name not in _default:
        _default[name] = k1_device.run(k1.case(name), k1.case(name).schedules[0])
    return _default[name]


def run_and_verify(variant, oracle, checker, name, schedule=None, kernel="auto"):
    """-> (the case, the variant's answer, what the rule measured)"""
    c = k1.case(name)
    schedule = schedule or c.schedules[0]
    answer = variant.run(c, schedule, kernel)
    backend = k1.VAR_WG if kernel == "workgroup" else k1.VAR
    return c, answer, k1.verify_pair(oracle, backend, name, schedule, answer, which=checker)


@pytest.mark.parametrize("shape", k1.SHAPE_IDS)
def test_every_workgroup_size(variant, oracle, checker, shape):
    """64-, 128-, 256-, 512- and 1024-lane workgroups of the reference-width build on odd image sizes, the middle frame ragged;
    the 520-patch frames split over four workgroups (svo_hip_sparse_align) and on one of 1024 lanes
    (svo_hip_sparse_align_workgroup), each against the checker and against each other"""
    name = "shape_" + shape
    answers = {kernel: run_and_verify(variant, oracle, checker, name, kernel=kernel)[1]
               for kernel in (("auto", "workgroup") if name in k1.WORKGROUP_TOO else ("auto",))}
    if name in k1.WORKGROUP_TOO:
        k1.verify_split(answers["auto"], answers["workgroup"])


def test_benchmark_instantiation(variant, oracle, checker):
    """sia_kernel<256, true, false>, VGA, 200 patches, levels 3 -> 0 (test_config2_vga_4levels)"""
    c, answer, m = run_and_verify(variant, oracle, checker, "vga16")
    assert se3.log_norm(answer.pose, c.batch.T_gt_w).max() < 5e-4


def test_variant_is_another_build_and_repeats_itself(variant):
    """the child did not run the default library under another name: on the 16 VGA pairs its poses differ in their bits from
    this process's default library, within the tolerance both hold against the oracle; and run twice it gives the same bits"""
    c = k1.case("vga16")
    v, dflt = variant.run(c, c.schedules[0]), default_of("vga16")
    assert not np.array_equal(v.pose.view(np.uint64), dflt.pose.view(np.uint64))
    assert se3.log_norm(v.pose, dflt.pose).max() <= k1.DEVICE.max_d
    again = variant.run(c, c.schedules[0], "again")
    for f in k1.FIELDS:
        assert np.array_equal(getattr(v, f).view(np.uint8), getattr(again, f).view(np.uint8)), f


@pytest.mark.parametrize("name", ["radtan_4to2", "radtan_3to0", "atan_4to2", "atan_3to0"])
def test_distorted_cameras(variant, oracle, checker, name):
    """the DIST instantiations, with the bounds of test_sparse_align_gpu.py::test_distorted_camera_models (which states no
    bound on the iteration sequences: under radtan the emulated kernels of BOTH widths part from the oracle's sequence by one
    last evaluation on one or two of these five frames, poses within 5e-6)"""
    kind, levels = name.split("_")
    schedule = {"4to2": (4, 2, 30), "3to0": (3, 0, 30)}[levels]
    c, answer, m = run_and_verify(variant, oracle, checker, f"{kind}_120", schedule)
    if levels == "3to0":
        assert se3.log_norm(answer.pose, c.batch.T_gt_w).max() < 1e-3   # both solved the problem


def test_distorted_camera_on_520_patches(variant, oracle, checker):
    """sia_kernel<256, false, true, 4> (svo_hip_sparse_align splits the frame) and sia_kernel<1024, false, true>, under the
    bounds of test_config3_xga5_n1000_parity: each against the checker, and against each other"""
    answers = {kernel: run_and_verify(variant, oracle, checker, "atan_520", kernel=kernel)[1] for kernel in ("auto", "workgroup")}
    k1.verify_split(answers["auto"], answers["workgroup"])


def test_ragged_and_missing_points(variant, oracle, checker):
    """n = 200, 12, 64, 65, 137, 0, 1"""
    c = k1.case("ragged")
    k1.verify_ragged(oracle, k1.VAR, variant.run(c, c.schedules[0]), which=checker)


def test_border_features_and_visibility(variant, oracle, checker):
    for schedule in k1.case("border").schedules:
        c, answer, m = run_and_verify(variant, oracle, checker, "border", schedule)
    assert np.all(answer.n_tracked < 200) and np.all(answer.n_tracked > 100), answer.n_tracked


def test_all_patches_outside(variant, oracle, checker):
    c = k1.case("outside")
    k1.verify_outside(oracle, k1.VAR, "outside", variant.run(c, c.schedules[0]), which=checker)


@pytest.mark.parametrize("n_iter", [0, 1, 2])
def test_iteration_caps(variant, oracle, checker, n_iter):
    run_and_verify(variant, oracle, checker, "itercap", (3, 0, n_iter))


def test_iteration_counts_on_256_problems(variant, oracle, checker):
    """16 pairs x 16 priors: >= 97 % identical per-level iteration sequences (the condition of
    test_iteration_counts_on_a_large_sample), tracked counts equal on those, every pose within 1e-4"""
    run_and_verify(variant, oracle, checker, "sample256")


@pytest.mark.parametrize("level", [3, 0])
def test_single_step(variant, oracle, checker, level):
    """ONE Gauss-Newton step at one level from a prior 5e-3 off (tests/test_sparse_align_emulated.py::
    test_emulated_single_gauss_newton_step): the f64 se3_exp and the products with nothing to correct them afterwards, to
    k1_cases.SINGLE_STEP_BOUND_GPU (with the figures it comes from)"""
    run_and_verify(variant, oracle, checker, f"step_level{level}")


def test_wave_kernel_is_the_same_code_in_both_libraries(variant, oracle, checker):
    """sparse_align_wave.hip does not read SIA_F64_PARTIALS: a batch of >= 1024 frames with <= 192 patches runs the f32-product
    wave-per-frame kernel in the reference-width library too (the benchmark's 200-patch headline does not take that path).
    Pinned down: on 32 pairs x 60 patches tiled to B = 1024 the variant's poses, iteration counts and H are the default
    library's bit for bit -- and hold the wave kernel's bounds against the checker."""
    c = k1.case("wave1024")
    v, dflt = variant.run(c, c.schedules[0]), default_of("wave1024")
    for f in ("pose", "iters", "H"):
        assert np.array_equal(getattr(v, f).view(np.uint8), getattr(dflt, f).view(np.uint8)), f
    assert np.array_equal(v.pose.reshape(32, 32, 12), np.broadcast_to(v.pose[:32], (32, 32, 12)))
    run_and_verify(variant, oracle, checker, "wave1024")
