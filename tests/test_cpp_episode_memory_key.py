"""Builds tests/cpp/episode_memory_key_test.cpp (g++, C++17; no library, no HIP) as a stand-alone program under AddressSanitizer and UBSan
and runs it: the episode memory's key order, digit selection, admission predicate, listing order, rank rule and merge rule
(gym.net_amd/csrc/episode_memory_key.hpp) against plain restatements.  A second run holds the same checks against the rules as they
stood before NaN returns and equal keys were specified: each of them must fail rows, or the checks prove nothing."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "episode_memory_key_test.cpp")
HEADER = os.path.join(ROOT, "gym.net_amd", "csrc", "episode_memory_key.hpp")
OUT_DIR = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(OUT_DIR, "episode_memory_key_test_san")
ENV = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(OUT_DIR, exist_ok=True)
    if not (os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in (SRC, HEADER))):
        # the sanitizer runtime is linked statically: the program runs in the inherited environment, whatever that preloads
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=undefined", "-static-libasan", SRC, "-o", EXE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    return EXE


def test_cpp_episode_memory_key_under_asan_and_ubsan(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"key: (\d+) checks, 0 failed", r.stdout)
    assert m and int(m.group(1)) > 1_000_000, r.stdout[-2000:]


def test_the_checks_fail_the_rules_as_they_were(exe):
    r = subprocess.run([exe, "--before"], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    failed = {name: int(n) for name, n in re.findall(r"before: (\S+) (\d+) failed", r.stdout)}
    assert set(failed) == {"predicate", "listing-order", "rank", "merge"} and all(n > 0 for n in failed.values()), r.stdout
