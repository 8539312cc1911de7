"""The log-probability a Discrete actor records (include/gymnet_amd.h, gymnet_vecenv_actor_act_logp_device) restated in C, operation for
operation in float32, compiled at test time with the host compiler (-ffp-contract=off) and called through ctypes, as
tests/_actor_softmax_twin.py restates the draw (helper module, not a conftest).  The arithmetic is specified, so the kernels of
actor_logp.hip are held to this twin's BITS: log_pos is csrc/log_pos.hpp's (the exponent and mantissa split by integer operations around
sqrt(2), a degree-8 Horner chain of fmaf, the exact sum of k * ln2_hi and f, one last addition), exp_neg is the softmax twin's with the
same constants, the sum S runs in index order, and logp = a_j - log_pos(S), the canonical NaN where S is not >= 1 or the result is a NaN.

exp_neg, draw, act, words and softmax64 come from tests/_actor_softmax_twin.py: the action a lane takes is that module's."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

import _actor_softmax_twin as stwin

exp_neg, draw, act, words, softmax64, inv_tau = stwin.exp_neg, stwin.draw, stwin.act, stwin.words, stwin.softmax64, stwin.inv_tau

OUT_DIR = stwin.OUT_DIR
SO = os.path.join(OUT_DIR, "actor_logp_twin.so")
F32 = np.float32
LOGP_BOUND = 2.0 ** -20
LOG_POS_BOUND = 2.0 ** -21
NAN_BITS = 0x7FC00000

_EXP_NEG_C = stwin.C_SRC[stwin.C_SRC.index("static const float kLog2e"):stwin.C_SRC.index("void exp_neg_twin")]

C_SRC = r"""
#include <math.h>
#include <stdint.h>
#include <string.h>
""" + _EXP_NEG_C + r"""
static const int32_t kSqrtHalfBits = 0x3f3504f3, kOneBits = 0x3f800000;
static const float ln2_hi = 0.693359375f, ln2_lo = -2.12194440e-4f;
static const float p0 = 7.0376836292e-2f, p1 = -1.1514610310e-1f, p2 = 1.1676998740e-1f, p3 = -1.2420140846e-1f, p4 = 1.4249322787e-1f,
                   p5 = -1.6668057665e-1f, p6 = 2.0000714765e-1f, p7 = -2.4999993993e-1f, p8 = 3.3333331174e-1f;
static float log_pos(float x) {
    int32_t i;
    memcpy(&i, &x, 4);
    i += kOneBits - kSqrtHalfBits;
    const float k = (float)((i >> 23) - 127);
    i = (i & 0x007fffff) + kSqrtHalfBits;
    float m;
    memcpy(&m, &i, 4);
    const float f = m - 1.0f;
    const float z = f * f;
    float p = p0;
    p = fmaf(p, f, p1);
    p = fmaf(p, f, p2);
    p = fmaf(p, f, p3);
    p = fmaf(p, f, p4);
    p = fmaf(p, f, p5);
    p = fmaf(p, f, p6);
    p = fmaf(p, f, p7);
    p = fmaf(p, f, p8);
    const float y = (f * z) * p;
    const float r = fmaf(-0.5f, z, y);
    const float hi = k * ln2_hi;
    const float s = hi + f;
    const float c = f - (s - hi);
    const float t = fmaf(k, ln2_lo, r) + c;
    return s + t;
}
void log_pos_twin(int64_t n, const float *x, float *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = log_pos(x[i]);
}
/* every float32 with a bit pattern in [lo, hi] (positive, ascending): the largest absolute error against the double log, how often a
   result is below its predecessor's (prev: the result before lo, or a NaN for none; the last result comes back in it), how many results
   are below +0 (a negative zero counts) */
void log_pos_sweep(uint32_t lo, uint32_t hi, float *prev, double *max_abs, int64_t *decreasing, int64_t *below_zero) {
    double wa = 0.0;
    int64_t dec = 0, neg = 0;
    float before = *prev;
    for (uint64_t b = lo; b <= hi; ++b) {
        const uint32_t w = (uint32_t)b;
        float x;
        memcpy(&x, &w, 4);
        const float g = log_pos(x);
        const double err = fabs((double)g - log((double)x));
        if (!(err <= wa)) wa = err;
        if (g < before) ++dec;
        if (!(g >= 0.0f) || signbit(g)) ++neg;
        before = g;
    }
    *prev = before; *max_abs = wa; *decreasing = dec; *below_zero = neg;
}
/* logits [n][A], action [n]; logp [n] out (bits) */
void logp_twin(int64_t n, int32_t A, const float *logits, float inv_tau, const int32_t *action, uint32_t *logp) {
    for (int64_t r = 0; r < n; ++r) {
        const float *x = logits + r * A;
        float m = x[0];
        for (int j = 1; j < A; ++j) if (x[j] > m) m = x[j];
        float a[8];
        float run = 0.0f;
        for (int j = 0; j < A; ++j) {
            const float d = x[j] - m;
            a[j] = d * inv_tau;
            run = run + exp_neg(a[j]);
        }
        uint32_t bits = 0x7FC00000u;
        if (run >= 1.0f) {
            const float lp = a[action[r]] - log_pos(run);
            if (lp == lp) memcpy(&bits, &lp, 4);
        }
        logp[r] = bits;
    }
}
"""

_lib = None
_lock = threading.Lock()


def lib():
    global _lib
    with _lock:
        if _lib is None:
            os.makedirs(OUT_DIR, exist_ok=True)
            src = os.path.join(OUT_DIR, "actor_logp_twin.c")
            if not os.path.exists(SO) or not os.path.exists(src) or open(src).read() != C_SRC:
                with open(src, "w") as f:
                    f.write(C_SRC)
                tmp = SO + f".{os.getpid()}.tmp"
                r = subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", tmp, "-lm"], capture_output=True, text=True)
                assert r.returncode == 0, r.stderr
                os.replace(tmp, SO)
            _lib = C.CDLL(SO)
            _lib.log_pos_twin.argtypes = [C.c_int64, C.c_void_p, C.c_void_p]
            _lib.log_pos_sweep.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
            _lib.logp_twin.argtypes = [C.c_int64, C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    return _lib


def log_pos(x):
    x = np.ascontiguousarray(x, F32)
    out = np.empty_like(x)
    lib().log_pos_twin(x.size, x.ctypes.data, out.ctypes.data)
    return out


def log_pos_sweep(lo_bits, hi_bits, prev=None):
    """(largest absolute error against the double log, results below their predecessor, results below +0, the last result) over every
    float32 whose bit pattern is in [lo_bits, hi_bits]; prev: the result of the argument before lo_bits (None: none)"""
    before = C.c_float(float("nan") if prev is None else float(prev))
    wa, dec, neg = C.c_double(), C.c_int64(), C.c_int64()
    lib().log_pos_sweep(int(lo_bits), int(hi_bits), C.byref(before), C.byref(wa), C.byref(dec), C.byref(neg))
    return wa.value, dec.value, neg.value, before.value


def logp(logits, actions, temperature):
    """uint32 [n]: the bits of logp for logits float32 [n, A] and the actions int32 [n] the lanes take, at the stored temperature"""
    logits = np.ascontiguousarray(logits, F32)
    n, A = logits.shape
    actions = np.ascontiguousarray(actions, np.int32)
    assert actions.shape == (n,) and 1 <= A <= 8 and ((actions >= 0) & (actions < A)).all()
    out = np.empty(n, np.uint32)
    lib().logp_twin(n, A, logits.ctypes.data, C.c_float(float(inv_tau(temperature))), actions.ctypes.data, out.ctypes.data)
    return out


def act_logp(logits, words_a, words_b, eps, explore="uniform", temperature=1.0):
    """(actions int32 [n], logp bits uint32 [n], explore mask, greedy) of one act call with logp under the setting"""
    actions, mask, greedy = act(logits, words_a, words_b, eps, explore, temperature)
    return actions, logp(logits, actions, temperature), mask, greedy


def log_softmax64(logits, temperature):
    """log softmax(logits / temperature) in float64 for the same float32 logits and the float32 temperature: [n, A]"""
    z = np.asarray(logits, F32).astype(np.float64) / float(F32(temperature))
    z = z - z.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))
