"""TEST INFRASTRUCTURE, not a test.  Usage: SVO_HIP_LIB=<library> python k1_width_child.py OUT.npz

rpg_svo_amd.capi binds its library when it is imported, so another build of it needs a process of its own: this one runs every
case of tests/k1_width_cases.py through helpers.run_hip on the library SVO_HIP_LIB names (the reference-width build of K1,
rpg_svo_amd/lib/variants/libsvo_hip_SIA_F64_PARTIALS.so, for tests/test_sparse_align_width_gpu.py) and writes pose, iters,
n_tracked, status, H and chi2 of each as "<case>/<kernel>/<field>", plus its wall time.  Nothing here catches an error of a
launch: the first one ends the process with a non-zero status."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


def run_case(name, kernel, out, tag=None):
    import k1_width_cases
    from helpers import run_hip
    b, (hi, lo, n_iter) = k1_width_cases.CASES[name]()
    T, res, _ = run_hip(b, hi, lo, n_iter, kernel=kernel)
    key = f"{name}/{tag or kernel}/"
    out[key + "pose"] = T
    for field in ("iters", "n_tracked", "status", "H", "chi2"):
        out[key + field] = getattr(res, field).cpu().numpy()


def main(path):
    t0 = time.perf_counter()
    from rpg_svo_amd import capi
    want = os.environ["SVO_HIP_LIB"]
    assert capi.lib_path() == want, (capi.lib_path(), want)
    capi.load()
    import k1_width_cases
    out = {}
    for name in k1_width_cases.CASES:
        run_case(name, "auto", out)
        if name in k1_width_cases.WORKGROUP_TOO:
            run_case(name, "workgroup", out)
        if name == k1_width_cases.TWICE:
            run_case(name, "auto", out, tag="again")
    wall = time.perf_counter() - t0
    out["wall_seconds"] = np.float64(wall)
    out["lib_path"] = np.array(capi.lib_path())
    np.savez(path, **out)
    print(f"k1_width_child: {len(k1_width_cases.CASES)} cases on {capi.lib_path()} in {wall:.1f} s")


if __name__ == "__main__":
    main(sys.argv[1])
