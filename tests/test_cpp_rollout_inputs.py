"""Builds tests/cpp/rollout_inputs_test.cpp (g++, C++17) and runs it: the refusals and the form picker of gymnet_rollout_inputs_device
(gym.net_amd/csrc/rollout_inputs.hpp, host-only and pure), as a stand-alone program that links nothing — once plain, once under
AddressSanitizer and UBSan with the sanitizer runtime linked statically.  Fails without the feature: the header does not exist."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "rollout_inputs_test.cpp")
CSRC = os.path.join(ROOT, "gym.net_amd", "csrc")


def _run(tmp_path, name, extra, env=None):
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + ["-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "rollout_inputs: 0 failed" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_cpp_refusals_and_picker_stand_alone(tmp_path):
    _run(tmp_path, "rollout_inputs_test", [])


def test_cpp_refusals_and_picker_under_asan_and_ubsan(tmp_path):
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    _run(tmp_path, "rollout_inputs_test_san", ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan"], env)
