"""A Discrete actor's softmax exploration (include/gymnet_amd.h, gymnet_vecenv_actor_set_exploration) restated in C, operation for operation
in float32, compiled at test time with the host compiler (-ffp-contract=off) and called through ctypes, as tests/_actor_twin.py restates
the forward pass (helper module, not a conftest).  The arithmetic is specified, so the kernels of actor_softmax.hip are held to this
twin's BITS: exp_neg is csrc/exp_neg.hpp's (one product by log2 e, rintf, a degree-7 Horner chain of fmaf, the exponent added as
integer bits; libm's fmaf rounds once like v_fma_f32, rintf rounds to nearest even like v_rndne_f32), the cumulative sums run in
index order, u = u01_24(word A), and the action is the first k with u * S < c_k, else the greedy one.

Beside it: the words of a lane from the NumPy Philox twin (oracle/numpy_ref.py), the coin (an integer compare with coin_threshold), the
uniform rule, and the same softmax in float64 in closed form — the yardstick the twin itself is held to in
tests/test_actor_softmax_host.py (its normalised cumulative distribution within 2^-20 of the float64 one)."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

from oracle import numpy_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_DIR = os.path.join(ROOT, "tests", "cpp", "build")
SO = os.path.join(OUT_DIR, "actor_softmax_twin.so")
F32 = np.float32
CDF_BOUND = 2.0 ** -20

C_SRC = r"""
#include <math.h>
#include <stdint.h>
#include <string.h>
static const float kLog2e = 1.44269504088896341f;
static const float c1 = 0.693147180559945309f, c2 = 0.240226506959100712f, c3 = 0.0555041086648215800f, c4 = 0.00961812910762847716f,
                   c5 = 0.00133335581464284434f, c6 = 0.000154035303933816099f, c7 = 0.0000152527338040598403f;
static float exp_neg(float a) {
    const float t = a * kLog2e;
    if (!(t >= -125.0f)) return 0.0f;
    const float n = rintf(t);
    const float f = t - n;
    float p = c7;
    p = fmaf(p, f, c6);
    p = fmaf(p, f, c5);
    p = fmaf(p, f, c4);
    p = fmaf(p, f, c3);
    p = fmaf(p, f, c2);
    p = fmaf(p, f, c1);
    p = fmaf(p, f, 1.0f);
    int32_t bits;
    memcpy(&bits, &p, 4);
    bits += (int32_t)n * (1 << 23);
    memcpy(&p, &bits, 4);
    return p;
}
void exp_neg_twin(int64_t n, const float *a, float *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = exp_neg(a[i]);
}
/* every float32 -x with the bit pattern of x in [lo, hi]: the largest absolute and relative error against the double exp */
void exp_neg_sweep(uint32_t lo, uint32_t hi, double *max_abs, double *max_rel) {
    double wa = 0.0, wr = 0.0;
    for (uint64_t b = lo; b <= hi; ++b) {
        const uint32_t w = (uint32_t)b | 0x80000000u;
        float a;
        memcpy(&a, &w, 4);
        const double want = exp((double)a), err = fabs((double)exp_neg(a) - want);
        if (err > wa) wa = err;
        if (err > wr * want) wr = err / want;
    }
    *max_abs = wa; *max_rel = wr;
}
/* logits [n][A], u [n]; greedy [n], cdf [n][A] (the c_k) and action [n] out */
void softmax_draw_twin(int64_t n, int32_t A, const float *logits, float inv_tau, const float *u, int32_t *greedy, float *cdf, int32_t *action) {
    for (int64_t r = 0; r < n; ++r) {
        const float *x = logits + r * A;
        int best = 0;
        float m = x[0];
        for (int j = 1; j < A; ++j) if (x[j] > m) { m = x[j]; best = j; }
        float run = 0.0f;
        for (int j = 0; j < A; ++j) {
            const float d = x[j] - m;
            const float a = d * inv_tau;
            run = run + exp_neg(a);
            cdf[r * A + j] = run;
        }
        const float thr = u[r] * run;
        int act = best;
        for (int j = A - 1; j >= 0; --j) if (thr < cdf[r * A + j]) act = j;
        greedy[r] = best;
        action[r] = act;
    }
}
"""

_lib = None
_lock = threading.Lock()                          # the sweep calls in from a thread pool: one build


def lib():
    global _lib
    with _lock:
        if _lib is None:
            os.makedirs(OUT_DIR, exist_ok=True)
            src = os.path.join(OUT_DIR, "actor_softmax_twin.c")
            if not os.path.exists(SO) or not os.path.exists(src) or open(src).read() != C_SRC:
                with open(src, "w") as f:
                    f.write(C_SRC)
                tmp = SO + f".{os.getpid()}.tmp"
                r = subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", tmp, "-lm"], capture_output=True, text=True)
                assert r.returncode == 0, r.stderr
                os.replace(tmp, SO)
            _lib = C.CDLL(SO)
            _lib.exp_neg_twin.argtypes = [C.c_int64, C.c_void_p, C.c_void_p]
            _lib.exp_neg_sweep.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
            _lib.softmax_draw_twin.argtypes = [C.c_int64, C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return _lib


def inv_tau(temperature):
    """1.0f / temperature, as the host computes it once"""
    return F32(1.0) / F32(temperature)


def exp_neg(a):
    a = np.ascontiguousarray(a, F32)
    out = np.empty_like(a)
    lib().exp_neg_twin(a.size, a.ctypes.data, out.ctypes.data)
    return out


def exp_neg_sweep(lo_bits, hi_bits):
    """(largest absolute, largest relative) error of exp_neg against the double exp over every float32 -x whose x has a bit pattern in
    [lo_bits, hi_bits]"""
    wa, wr = C.c_double(), C.c_double()
    lib().exp_neg_sweep(int(lo_bits), int(hi_bits), C.byref(wa), C.byref(wr))
    return wa.value, wr.value


def draw(logits, u, temperature):
    """(action int32 [n], greedy int32 [n], c float32 [n, A]) of the softmax draw for logits float32 [n, A] and u float32 [n]"""
    logits = np.ascontiguousarray(logits, F32)
    n, A = logits.shape
    u = np.ascontiguousarray(u, F32)
    assert u.shape == (n,) and 1 <= A <= 8
    greedy, action, cdf = np.empty(n, np.int32), np.empty(n, np.int32), np.empty((n, A), F32)
    lib().softmax_draw_twin(n, A, logits.ctypes.data, C.c_float(float(inv_tau(temperature))), u.ctypes.data, greedy.ctypes.data, cdf.ctypes.data,
                            action.ctypes.data)
    return action, greedy, cdf


def coin_threshold(eps):
    """philox.hpp coin_threshold: u01_24(w) <= epsilon exactly when w <= this (epsilon * 2^24 is exact in float32)"""
    t = np.floor(np.float64(F32(eps)) * 16777216.0)
    if not t >= 0:
        return 0
    return 0xFFFFFFFF if t >= 16777215.0 else (int(t) << 8) | 0xFF


def words(seed, lane0, tick, n):
    """(A, B) uint32 [n] of global lanes lane0 .. lane0 + n - 1 at (seed, tick)"""
    lanes = np.uint64(int(lane0)) + np.arange(n, dtype=np.uint64)
    return numpy_ref.action_words(int(seed) & 0xFFFFFFFFFFFFFFFF, lanes, int(tick))


def explore_mask(words_b, eps):
    return np.asarray(words_b, np.uint32) <= np.uint32(coin_threshold(eps))


def uniform(words_a, A):
    """Discrete.Sample(): umulhi(word A, A)"""
    return ((np.asarray(words_a, np.uint32).astype(np.uint64) * np.uint64(A)) >> np.uint64(32)).astype(np.int32)


def act(logits, words_a, words_b, eps, explore="softmax", temperature=1.0, u_words=None):
    """(actions int32 [n], explore mask, greedy) of one act call under the setting (explore, temperature).  u_words: the words u is taken
    from instead of word A (the statistics test passes word B to show why that would be wrong)."""
    logits = np.ascontiguousarray(logits, F32)
    mask = explore_mask(words_b, eps)
    u = numpy_ref.u01_24(np.asarray(words_a if u_words is None else u_words, np.uint32))
    drawn, greedy, _ = draw(logits, u, temperature)
    if explore == "uniform":
        drawn = uniform(words_a, logits.shape[1])
    else:
        assert explore == "softmax"
    return np.where(mask, drawn, greedy).astype(np.int32), mask, greedy


def softmax64(logits, temperature):
    """softmax(logits / temperature) in float64 for the same float32 logits and the float32 temperature: probabilities [n, A]"""
    z = np.asarray(logits, F32).astype(np.float64) / float(F32(temperature))
    z = z - z.max(axis=1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(axis=1, keepdims=True)
