"""The Box actor's log-density (gym.net_amd/csrc/actor_box_logd.hip, gymnet_vecenv_actor_box_act_logd_device) restated in NumPy float32,
operation by operation (helper module, not a conftest):

    inv_sigma = float32(1.0 / float64(sigma))
    c         = float32(-log(float64(sigma)) - ln(2 pi) / 2)
    d    = (a - g) * inv_sigma        each operation rounded to float32
    h    = -0.5f * d
    logd = fmaf(h, d, c)

The fmaf is the float64 product (exact: two 24-bit significands) plus c, rounded once to float32.  The float64 sum is itself rounded, so
where it lands within one float64 step of a float32 rounding boundary the lane is decided exactly, over rationals: the twin rounds once,
as the instruction does.  c and inv_sigma come from float64; for the sigmas the tests use, math.log and np.log give the same float32 c
(asserted at import)."""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
HALF_LN_2PI = 0.91893853320467274178
SIGMAS = (0.25, 0.5, 0.3, 1.7)


def constants(sigma):
    """(inv_sigma, c) float32 of the float32 sigma"""
    s = float(F32(sigma))
    return F32(1.0 / s), F32(-math.log(s) - HALF_LN_2PI)


for _s in SIGMAS:
    assert constants(_s)[1].view(np.uint32) == F32(-np.log(np.float64(F32(_s))) - np.float64(HALF_LN_2PI)).view(np.uint32), _s


def _fma(h, d, c):
    """float32 fmaf(h, d, c) of float32 arrays h, d and the float32 scalar c"""
    with np.errstate(over="ignore", invalid="ignore"):
        s = h.astype(np.float64) * d.astype(np.float64) + np.float64(c)
        out = s.astype(F32)
        near = np.isfinite(s) & (np.nextafter(s, -np.inf).astype(F32) != np.nextafter(s, np.inf).astype(F32))
    for k in np.nonzero(near)[0]:                                            # (rare: about one lane in 2^28)
        lo, hi = np.nextafter(s[k], -np.inf).astype(F32), np.nextafter(s[k], np.inf).astype(F32)
        if not (np.isfinite(lo) and np.isfinite(hi)):
            continue
        exact = Fraction(float(h[k])) * Fraction(float(d[k])) + Fraction(float(c))
        mid = (Fraction(float(lo)) + Fraction(float(hi))) / 2
        even = lo if (int(lo.view(np.uint32)) & 1) == 0 else hi
        out[k] = hi if exact > mid else (lo if exact < mid else even)
    return out


def logd(a, g, sigma):
    """float32 [n]: the log-density of the actions a around the greedy actions g at sigma"""
    inv, c = constants(sigma)
    a, g = np.asarray(a, F32).reshape(-1), np.asarray(g, F32).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        d = ((a - g).astype(F32) * inv).astype(F32)
        h = (F32(-0.5) * d).astype(F32)
    return _fma(h, d, c)


def logd64(a, g, sigma):
    """(the float64 closed form -d^2 / 2 - ln sigma - ln(2 pi) / 2 of the same float32 inputs, d^2)"""
    s = np.float64(F32(sigma))
    d = (np.asarray(a, F32).astype(np.float64) - np.asarray(g, F32).astype(np.float64)) / s
    return -0.5 * d * d - np.log(s) - HALF_LN_2PI, d * d
