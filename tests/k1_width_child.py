"""TEST INFRASTRUCTURE, not a test.  Usage: SVO_HIP_LIB=<library> python k1_width_child.py OUT.npz

rpg_svo_amd.capi binds its library when it is imported, so another build of it needs a process of its own: this one runs the
variant pairs of tests/k1_cases.py's table through tests/k1_device.py on the library SVO_HIP_LIB names (the reference-width build
of K1, rpg_svo_amd/lib/variants/libsvo_hip_SIA_F64_PARTIALS.so, for tests/test_sparse_align_width_gpu.py) and writes the
K1Answer of each as "<case>/<schedule>/<auto|workgroup|again>/<field>", plus its wall time.  Nothing here catches an error of a
launch: the first one ends the process with a non-zero status."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

KERNELS = {"var": ("auto", "auto"), "var_wg": ("workgroup", "workgroup"), "var_twice": ("again", "auto")}   # backend -> (tag, kernel)


def key(name, schedule, tag):
    return f"{name}/{'-'.join(map(str, schedule))}/{tag}/"


def main(path):
    t0 = time.perf_counter()
    from rpg_svo_amd import capi
    want = os.environ["SVO_HIP_LIB"]
    assert capi.lib_path() == want, (capi.lib_path(), want)
    capi.load()
    import k1_cases
    import k1_device
    out, n = {}, 0
    for backend, (tag, kernel) in KERNELS.items():
        for name in k1_cases.cases_of(backend):
            for schedule in k1_cases.schedules_of(name, backend):
                answer = k1_device.run(k1_cases.case(name), schedule, kernel)
                out.update({key(name, schedule, tag) + f: a for f, a in answer._asdict().items()})
                n += 1
    wall = time.perf_counter() - t0
    out["wall_seconds"] = np.float64(wall)
    out["lib_path"] = np.array(capi.lib_path())
    np.savez(path, **out)
    print(f"k1_width_child: {n} runs on {capi.lib_path()} in {wall:.1f} s")


if __name__ == "__main__":
    main(sys.argv[1])
