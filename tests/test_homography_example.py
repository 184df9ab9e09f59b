"""examples/homography_init.cpp: the bootstrap's homography step through the C ABI from plain C++ -- builds with g++ against
the library (no GPU needed), and on the device recovers the pose of a synthetic two-view scene and a point cloud whose
median depth is the map scale."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "homography_init")


def _build():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    lib = os.path.join(ROOT, "rpg_svo_amd", "lib")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "homography_init.cpp"),
                    "-L", lib, "-lsvo_hip", f"-Wl,-rpath,{lib}", "-o", EXE], check=True)


def test_homography_example_builds(hip_lib):
    _build()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_homography_example_recovers_the_pose(hip_lib, gpu_device):
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "OK" in r.stdout
