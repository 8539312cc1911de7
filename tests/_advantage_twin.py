"""gymnet_gae_device's recurrence (include/gymnet_amd.h) restated in C with libm's fmaf, compiled at test time with the host compiler and
called through ctypes, in the manner of _actor_twin.py: per lane, t = T-1 .. 0, carrying A and vnext,
    nv = (d & 1) ? +0 : (d & 2) ? (boot ? boot[t] : +0) : vnext;  delta = fmaf(gamma, nv, r) - v;  A = d ? delta : fmaf(gl, A, delta);
    advantage = A;  return = A + v;  vnext = v
with gl = gamma * lambda one float32 product.  fmaf rounds once, like v_fma_f32, and -ffp-contract=off keeps every other operation apart, so
the GPU tests compare bits.
gae64 is the same quantity written the other way round in float64 NumPy — A_t = sum_k (gamma lambda)^k delta_{t+k} up to and including the first cut at or after row t, all lanes
at once — so that a slip in the twin's control flow does not repeat itself there.
case(), NS, WIDE_NS and steps_for are the inputs tests/test_gpu_advantage.py runs; tests/test_advantage_host.py holds the twin to gae64 over the same."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_DIR = os.path.join(ROOT, "tests", "cpp", "build")
SO = os.path.join(OUT_DIR, "advantage_twin.so")
F32 = np.float32

C_SRC = r"""
#include <math.h>
#include <stdint.h>
/* rows of `stride` elements, lane i = column i; any of v, vlast, boot, adv, ret may be NULL.  Each element is read before the same
   element of an output is written, so adv / ret may be r / v */
void advantage_twin(int64_t T, int64_t n, int64_t stride, const float *r, const uint8_t *d, const float *v, const float *vlast,
                    const float *boot, float gamma, float lambda, float *adv, float *ret) {
    const float gl = gamma * lambda;
    for (int64_t i = 0; i < n; ++i) {
        float A = 0.0f, vnext = vlast ? vlast[i] : 0.0f;
        for (int64_t t = T - 1; t >= 0; --t) {
            const int64_t k = t * stride + i;
            const uint8_t dk = d[k];
            const float rk = r[k], vk = v ? v[k] : 0.0f, bk = boot ? boot[k] : 0.0f;
            const float nv = (dk & 1) ? 0.0f : (dk & 2) ? bk : vnext;
            const float delta = fmaf(gamma, nv, rk) - vk;
            A = dk ? delta : fmaf(gl, A, delta);
            if (adv) adv[k] = A;
            if (ret) ret[k] = A + vk;
            vnext = vk;
        }
    }
}
"""

_lib = None


def lib():
    global _lib
    if _lib is None:
        os.makedirs(OUT_DIR, exist_ok=True)
        src = os.path.join(OUT_DIR, "advantage_twin.c")
        if not os.path.exists(SO) or not os.path.exists(src) or open(src).read() != C_SRC:
            with open(src, "w") as f:
                f.write(C_SRC)
            tmp = SO + f".{os.getpid()}.tmp"
            r = subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", tmp, "-lm"], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            os.replace(tmp, SO)
        _lib = C.CDLL(SO)
        _lib.advantage_twin.argtypes = [C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 5 + [C.c_float, C.c_float, C.c_void_p, C.c_void_p]
        _lib.advantage_twin.restype = None
    return _lib


def gae(r, d, v=None, vlast=None, boot=None, gamma=0.99, lam=0.95):
    """(advantage, return) float32 [T, n] of contiguous r float32 [T, n], d uint8 [T, n], v / boot float32 [T, n] or None, vlast [n] or None"""
    r = np.ascontiguousarray(r, F32)
    T, n = r.shape
    d = np.ascontiguousarray(d, np.uint8)
    keep = [None if x is None else np.ascontiguousarray(x, F32) for x in (v, vlast, boot)]
    assert d.shape == (T, n) and all(x is None or x.shape == s for x, s in zip(keep, ((T, n), (n,), (T, n))))
    adv, ret = np.empty((T, n), F32), np.empty((T, n), F32)
    lib().advantage_twin(T, n, n, r.ctypes.data, d.ctypes.data, *[None if x is None else x.ctypes.data for x in keep], gamma, lam,
                         adv.ctypes.data, ret.ctypes.data)
    return adv, ret


def gae64(r, d, v=None, vlast=None, boot=None, gamma=0.99, lam=0.95):
    """the same in float64, as a forward sum per episode segment: A_t = sum_{k >= 0} (gamma lam)^k delta_{t+k} over the rows t .. the first
    row at or after t whose done byte is set (or T-1).  gamma and lam are taken as the float32 values the kernel is handed"""
    r = np.asarray(r, np.float64)
    T, n = r.shape
    d = np.asarray(d, np.uint8)
    v = np.zeros((T, n)) if v is None else np.asarray(v, np.float64)
    vlast = np.zeros(n) if vlast is None else np.asarray(vlast, np.float64)
    boot = np.zeros((T, n)) if boot is None else np.asarray(boot, np.float64)
    g, gl = float(F32(gamma)), float(F32(gamma)) * float(F32(lam))
    vnext = np.concatenate([v[1:], vlast[None]], axis=0)
    nv = np.where(d & 1, 0.0, np.where(d & 2, boot, vnext))
    delta = r + g * nv - v
    adv = np.zeros((T, n))
    for t in range(T):
        alive, w = np.ones(n, bool), 1.0                             # alive: no cut in rows t .. t + k - 1
        for k in range(T - t):
            adv[t] += np.where(alive, w * delta[t + k], 0.0)
            alive &= d[t + k] == 0
            w *= gl
            if not alive.any():
                break
    return adv, adv + v


NS = (1, 3, 4, 252, 1028, 1030)         # a single thread; a partial wave; a ragged tail; a second block (V = 1 at these counts: advantage.hpp)
WIDE_NS = (1 << 18, (1 << 18) + 4, (1 << 18) + 252)    # V = 4 runs from 2^18 lanes: whole blocks; a last block of one thread; a partial last wave
WIDE_T = 9                                             # the row count at which the wide lane counts run every form and layout


def steps_for(us):
    """the row counts around the U rows in flight of each V: T in {1, 2, U-1, U, U+1, 2U+1, 33} for every U in `us`"""
    return tuple(sorted({1, 2, 33} | {t for u in us for t in (u - 1, u, u + 1, 2 * u + 1)}))


def case(T, n, seed=0):
    """dict(r, d, v [T + 1, n] (row T = last value), boot): dones at rate ~0.1 with bytes from {1, 2, 3}, and a done planted on rows 0 and
    T-1 (lanes 0 mod 3 and 1 mod 3; with n = 1 lane 0 gets row 0, and row T-1 too where T > 1)"""
    rng = np.random.default_rng([seed, T, n])
    r = rng.standard_normal((T, n)).astype(F32)
    v = rng.standard_normal((T + 1, n)).astype(F32)
    boot = rng.standard_normal((T, n)).astype(F32)
    d = np.where(rng.random((T, n)) < 0.1, rng.integers(1, 4, (T, n)), 0).astype(np.uint8)
    lanes = np.arange(n)
    d[0, lanes % 3 == 0] = rng.integers(1, 4, int((lanes % 3 == 0).sum()))
    d[T - 1, lanes % 3 == 1] = rng.integers(1, 4, int((lanes % 3 == 1).sum()))
    if n == 1 and T > 1:
        d[T - 1, 0] = 2
    return {"r": r, "d": d, "v": v, "boot": boot}


def same(a, b):
    """bit equality of float32 arrays, except that a NaN matches any NaN (the payload is not compared)"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
