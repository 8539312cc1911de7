"""Builds tests/cpp/rollout_plan_boot_test.cpp (g++, C++17; no library, no HIP) and runs it: the boot request (V(terminal observation) on
time-limit rows) in the fused rollout's plan (gym.net_amd/csrc/rollout_plan.hpp) — every new refusal for a Discrete and for a Box actor, its
status, text and order relative to the existing ones, and requests without a boot pointer planned as before with the new fields at their
defaults.  Fails without the feature: FusedRequest has no rec_boot and FusedFacts no max_episode_steps."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "rollout_plan_boot_test.cpp")
HEADER = os.path.join(ROOT, "gym.net_amd", "csrc", "rollout_plan.hpp")
OUT_DIR = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(OUT_DIR, "rollout_plan_boot_test")


def test_cpp_rollout_plan_boot_table():
    os.makedirs(OUT_DIR, exist_ok=True)
    deps = [SRC, HEADER, os.path.join(ROOT, "include", "gymnet_amd.h")]
    if not (os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps)):
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", SRC, "-o", EXE], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "100 rows, 0 failed" in r.stdout, r.stdout
