"""The actor's forward pass restated in C with fmaf (include/gymnet_amd.h, gymnet_vecenv_actor_config), compiled at test time with the
host compiler and called through ctypes: neuron j of layer l is acc = b[j]; acc = fmaf(W[j][i], x[i], acc) for ascending i, hidden
layers take acc > 0 ? acc : +0.0f, the action is the first index of the largest logit.  libm's fmaf rounds once, like v_fma_f32.
Also the history rules (config / reset fill every slot, push appends or refills) and the epsilon-greedy composition, in NumPy, and
the (W, b) pairs of a flat weight block (layers / net) that the GPU tests hand to VectorEnv.Actor."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_DIR = os.path.join(ROOT, "tests", "cpp", "build")
SO = os.path.join(OUT_DIR, "actor_twin.so")

C_SRC = r"""
#include <math.h>
#include <stdint.h>
void actor_twin(int64_t n, int32_t layers, const int32_t *widths, const float *weights, const float *x, float *logits, int32_t *greedy) {
    float a[64], b[64];
    for (int64_t r = 0; r < n; ++r) {
        for (int i = 0; i < widths[0]; ++i) a[i] = x[r * widths[0] + i];
        const float *p = weights;
        for (int l = 0; l < layers; ++l) {
            const int win = widths[l], wout = widths[l + 1];
            const float *W = p, *bias = p + (int64_t)wout * win;
            for (int j = 0; j < wout; ++j) {
                float acc = bias[j];
                for (int i = 0; i < win; ++i) acc = fmaf(W[j * win + i], a[i], acc);
                b[j] = (l + 1 < layers) ? (acc > 0.0f ? acc : 0.0f) : acc;
            }
            for (int j = 0; j < wout; ++j) a[j] = b[j];
            p += (int64_t)wout * win + wout;
        }
        const int nout = widths[layers];
        int best = 0;
        for (int j = 0; j < nout; ++j) {
            logits[r * nout + j] = a[j];
            if (j > 0 && a[j] > a[best]) best = j;
        }
        greedy[r] = best;
    }
}
"""

_lib = None


def lib():
    global _lib
    if _lib is None:
        os.makedirs(OUT_DIR, exist_ok=True)
        src = os.path.join(OUT_DIR, "actor_twin.c")
        if not os.path.exists(SO) or not os.path.exists(src) or open(src).read() != C_SRC:
            with open(src, "w") as f:
                f.write(C_SRC)
            tmp = SO + f".{os.getpid()}.tmp"
            r = subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", tmp, "-lm"], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            os.replace(tmp, SO)
        _lib = C.CDLL(SO)
        _lib.actor_twin.argtypes = [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return _lib


def forward(widths, flat, x):
    """(logits float32 [n, w_L], greedy int32 [n]) for x float32 [n, w_0]."""
    widths = np.ascontiguousarray(widths, np.int32)
    flat = np.ascontiguousarray(flat, np.float32)
    x = np.ascontiguousarray(x, np.float32).reshape(-1, int(widths[0]))
    n = x.shape[0]
    logits = np.empty((n, int(widths[-1])), np.float32)
    greedy = np.empty(n, np.int32)
    lib().actor_twin(n, len(widths) - 1, widths.ctypes.data, flat.ctypes.data, x.ctypes.data, logits.ctypes.data, greedy.ctypes.data)
    return logits, greedy


def forward64(widths, flat, x):
    """The same network in float64 (no fma), and sum |W x| + |b| per neuron of the last layer: the rounding bound's scale."""
    a = np.asarray(x, np.float64).reshape(-1, int(widths[0]))
    absa = np.abs(a)
    p = 0
    L = len(widths) - 1
    for l in range(L):
        win, wout = int(widths[l]), int(widths[l + 1])
        W = np.asarray(flat[p:p + wout * win], np.float64).reshape(wout, win)
        b = np.asarray(flat[p + wout * win:p + wout * win + wout], np.float64)
        p += wout * win + wout
        z = a @ W.T + b
        scale = absa @ np.abs(W).T + np.abs(b)
        a = np.maximum(z, 0.0) if l + 1 < L else z
        absa = scale
    return a, absa


def random_net(rng, widths, scale=1.0):
    flat = []
    for l in range(len(widths) - 1):
        win, wout = widths[l], widths[l + 1]
        flat.append(rng.normal(0, scale / np.sqrt(win), (wout, win)).astype(np.float32).ravel())
        flat.append(rng.normal(0, 0.1, wout).astype(np.float32))
    return np.asarray(widths, np.int32), np.concatenate(flat).astype(np.float32)


def layers(widths, flat):
    """The (W [out][in], b [out]) pairs of a flat block in gymnet_vecenv_actor_config's layout: what VectorEnv.Actor takes."""
    pairs, p = [], 0
    for l in range(len(widths) - 1):
        win, wout = int(widths[l]), int(widths[l + 1])
        pairs.append((flat[p:p + win * wout].reshape(wout, win), flat[p + win * wout:p + win * wout + wout]))
        p += win * wout + wout
    assert p == len(flat)
    return pairs


def net(rng, widths, scale=2.0):
    """(widths int32, flat float32, (W, b) pairs) of a random network."""
    w, flat = random_net(rng, widths, scale=scale)
    return w, flat, layers(widths, flat)


def same(a, b):
    """bit equality of float32 arrays with -0 == +0 (the sign of a zero sum is the one thing the kernel's zero padding may change)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.array_equal(a == 0, b == 0) and np.array_equal(np.where(a == 0, 0, a).view(np.uint32), np.where(b == 0, 0, b).view(np.uint32))


def compose(greedy, sampled_or_none, explore):
    return np.where(explore, sampled_or_none, greedy).astype(np.int32)


class History:
    """The history rules on the host: [N, S, O] oldest first."""

    def __init__(self, obs, S):
        obs = np.asarray(obs, np.float32)
        self.h = np.repeat(obs[:, None, :], S, axis=1)

    def reset(self, obs, mask=None):
        obs = np.asarray(obs, np.float32)
        m = np.ones(len(obs), bool) if mask is None else np.asarray(mask) != 0
        self.h[m] = obs[m][:, None, :]

    def push(self, obs, done):
        obs = np.asarray(obs, np.float32)
        d = np.asarray(done) != 0
        self.h = np.concatenate([self.h[:, 1:], obs[:, None, :]], axis=1)
        self.h[d] = obs[d][:, None, :]

    def x(self):
        return self.h.reshape(len(self.h), -1)
