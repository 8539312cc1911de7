"""Builds tests/cpp/actor_box_policy_test.cpp (g++, C++17) against include/gymnet_amd.hpp, libgymnet_amd.so and the HIP runtime and runs
it: the C++ host methods of a Box actor's policy (SetBoxActorPolicy / GetBoxActorPolicy)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "actor_box_policy_test.cpp")
OUT_DIR = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(OUT_DIR, "actor_box_policy_test")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def _build(gymnet):
    lib_dir = os.path.dirname(gymnet.LIB_PATH)
    os.makedirs(OUT_DIR, exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "include", "gymnet_amd.hpp"), os.path.join(ROOT, "include", "gymnet_amd.h"), gymnet.LIB_PATH]
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps):
        return EXE
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROCM, "include"), SRC, "-o", EXE, "-L", lib_dir, "-lgymnet_amd", "-L", os.path.join(ROCM, "lib"), "-lamdhip64",
           f"-Wl,-rpath,{lib_dir}", f"-Wl,-rpath,{os.path.join(ROCM, 'lib')}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return EXE


def test_cpp_actor_box_policy_cpu(gymnet):
    exe = _build(gymnet)
    r = subprocess.run([exe, "--cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpu: 0 failed" in r.stdout


@pytest.mark.gpu
def test_cpp_actor_box_policy_gpu(gpu_pkg):
    exe = _build(gpu_pkg)
    r = subprocess.run([exe, "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpu+gpu: 0 failed" in r.stdout
