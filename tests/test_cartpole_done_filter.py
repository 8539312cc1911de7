"""The exact float32 pre-filter of CartPole's done flag (gym.net_amd/csrc/cartpole_done_filter.hpp, used by the headline step kernel's
full-workgroup body: docs/ledger.md §38), on the CPU: tests/cpp/cartpole_done_filter_test.cpp built with g++ -ffp-contract=off (the
product's rounding contract: product, then sum).

  * sweeps: every float32 position within 64 steps of +-x_threshold and +-theta_threshold against a velocity grid (0, +-denormal, +-tiny,
    +-large, +-max, NaN, +-inf, and velocities that bring the sum back to zero or to the other threshold); positions well inside (and NaN,
    infinite, far outside) with velocities that put the SUM within 64 steps of a threshold; the grid against itself.  Wherever the filter
    decides a term its flag is the binary64 expression's; it never decides wrongly, and it is not vacuous (it decides some and leaves some);
  * the 3200 reference-text vectors (tests/golden/cartpole_reference_text.npz; 200 of them within +-2 float32 ulps of a threshold): the
    flag "filter where it decides, binary64 where it does not" is the reference's on every vector, and every vector whose flag a plain
    float32 compare of the float32 sums would flip — 22 of them — has its term in the ambiguous band.  That is a condition on the band."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "cartpole_done_filter_test.cpp")
CSRC = os.path.join(ROOT, "gym.net_amd", "csrc")
OUT_DIR = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(OUT_DIR, "cartpole_done_filter_test")
FLIPPING = 22


@pytest.fixture(scope="module")
def exe():
    os.makedirs(OUT_DIR, exist_ok=True)
    deps = [SRC, os.path.join(CSRC, "cartpole_done_filter.hpp")]
    if not (os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps)):
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-I", CSRC, SRC, "-o", EXE], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    return EXE


def test_filter_never_decides_wrongly_on_the_sweeps(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "filter never decides wrongly" in r.stdout and "WRONG" not in r.stdout


def test_reference_text_vectors_come_out_as_the_reference_and_the_flipping_ones_are_ambiguous(exe):
    g = np.load(os.path.join(ROOT, "tests", "golden", "cartpole_reference_text.npz"))
    s = g["state"].astype(np.float32)
    assert np.array_equal(s.astype(np.float64), g["state"])                       # the inputs ARE float32 values
    text = "\n".join(" ".join("%08x" % int(b) for b in s[:, i].view(np.uint32)) for i in range(s.shape[1])) + "\n"
    r = subprocess.run([exe, "eval"], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    t = np.array([[int(v) for v in l.split()] for l in r.stdout.strip().split("\n")], dtype=bool)
    assert t.shape == (s.shape[1], 6)
    dec_x, flag_x, exact_x, dec_t, flag_t, exact_t = t.T
    done = g["done"].astype(bool)
    assert np.array_equal(exact_x | exact_t, done)                                 # the binary64 expression is the reference's flag
    assert np.array_equal(np.where(dec_x, flag_x, exact_x) | np.where(dec_t, flag_t, exact_t), done)
    assert not (dec_x & (flag_x != exact_x)).any() and not (dec_t & (flag_t != exact_t)).any()
    # what plain float32 compares of the float32 sums would answer, term by term
    tau = np.float32(0.02)
    with np.errstate(invalid="ignore", over="ignore"):
        nx, nt = s[0] + tau * s[1], s[2] + tau * s[3]
        naive_x, naive_t = np.abs(nx) > np.float32(2.4), np.abs(nt) > np.float32(0.20943951606750488)
    flips = (naive_x | naive_t) != done
    print("flipping vectors:", int(flips.sum()), "ambiguous x terms:", int((~dec_x).sum()), "ambiguous theta terms:", int((~dec_t).sum()))
    assert int(flips.sum()) >= FLIPPING
    assert not (dec_x & (naive_x != exact_x)).any() and not (dec_t & (naive_t != exact_t)).any()     # a flipping TERM is never decided
    assert (~dec_x | ~dec_t)[flips].all()                                                            # so every flipping vector is in the band
    # the fixture's in-range block (positions inside both thresholds, sums away from them) is decided: the filter is not vacuous here either
    with np.errstate(invalid="ignore"):
        calm = (np.abs(s[0]) < 2.0) & (np.abs(nx) < 2.0) & (np.abs(s[2]) < 0.2) & (np.abs(nt) < 0.2)
    assert calm.sum() > 100 and (dec_x & dec_t)[calm].all()
