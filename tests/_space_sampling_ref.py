"""A plain float64 reference of the stand-alone space samplers (csrc/kernels.hip: sample_box_kernel, sample_box_elementwise_kernel,
sample_discrete_kernel, sample_discrete_masked_kernel, compose_discrete_kernel), element by element.

The only thing taken from the oracle is the pair of Philox words of a lane, `oracle.action_words(key, lane0, tick, count)` -> (A, B);
every value is then computed here in NumPy float64 / Python integers, in the closed form Box.cs:82-85, Discrete.cs:17-28 and
TrainingPlaySession.cs:46-52 state — not in the float32 operation order of the kernel.  Shared by tests/test_space_sampling_host.py
(which holds it against the C oracle where the two overlap) and tests/test_gpu_space_sampling.py (which holds the kernels against it).
"""
import numpy as np

MASK64 = (1 << 64) - 1
ELEMENT_KEY_STEP = 0xD1B54A32D192ED03      # element e of the elementwise sampler draws from key seed + e * this (mod 2^64)
TWO24 = 16777216.0
FLT_MAX = float(np.finfo(np.float32).max)

# Global lanes whose words are extreme, for (seed, tick) = (EXTREME_SEED, EXTREME_TICK): found once by find_extreme_lanes() below
# over lanes [0, 2^27) (the first two of each kind); tests/test_space_sampling_host.py re-derives every one from the oracle.
EXTREME_SEED, EXTREME_TICK = 7, 1
A_ZERO = (5166529, 10075959)               # word A >> 8 == 0:        u == 0, u1 == 2^-24 (the smallest)
A_MAX = (1494407, 10480431)                # word A >> 8 == 0xFFFFFF: u == 1 - 2^-24 (the largest), u1 == 1
B_ZERO = (29821414, 91483721)              # word B >> 8 == 0:        the coin / u2 == 0
B_MAX = (15266732, 38359651)               # word B >> 8 == 0xFFFFFF: the coin / u2 == 1 - 2^-24
WINDOW = 8                                 # lanes per window around an extreme lane
WINDOW_LEAD = 3                            # a window starts this many lanes before its extreme lane: inside a group of four


def extreme_windows():
    """[(first lane, extreme lane)] of the WINDOW-lane windows around every committed extreme lane."""
    return [(lane - WINDOW_LEAD, lane) for lane in A_ZERO + A_MAX + B_ZERO + B_MAX]


def find_extreme_lanes(oracle, seed=EXTREME_SEED, tick=EXTREME_TICK, lanes=1 << 27, chunk=1 << 22):
    """The search that produced the constants above (about 8 s; no test calls it): every lane in [0, lanes) with an extreme word."""
    found = {"A_ZERO": [], "A_MAX": [], "B_ZERO": [], "B_MAX": []}
    for lane0 in range(0, lanes, chunk):
        a, b = oracle.action_words(seed, lane0, tick, min(chunk, lanes - lane0))
        for name, w, top in (("A_ZERO", a, 0), ("A_MAX", a, 0xFFFFFF), ("B_ZERO", b, 0), ("B_MAX", b, 0xFFFFFF)):
            found[name] += [lane0 + int(i) for i in np.nonzero((w >> 8) == top)[0]]
    return found


def element_key(seed, element):
    return (int(seed) + int(element) * ELEMENT_KEY_STEP) & MASK64


def words(oracle, seed, lane0, tick, count, element=0):
    """Words (A, B) of `count` lanes from global lane `lane0`, for element `element` of the elementwise sampler (0: the scalar one)."""
    return oracle.action_words(element_key(seed, element), int(lane0), int(tick), int(count))


def uniforms(a, b):
    """u in [0, 1), u1 in (0, 1] (both from word A) and u2 in [0, 1) (word B), float64 and exact."""
    top = (np.asarray(a, dtype=np.uint32) >> 8).astype(np.float64)
    return top / TWO24, (top + 1.0) / TWO24, (np.asarray(b, dtype=np.uint32) >> 8).astype(np.float64) / TWO24


def box_sample(low, high, a, b):
    """Box.Sample() of one element with float32 bounds (low, high) for the lanes whose words are (a, b): Box.cs:82-85."""
    low, high = float(np.float32(low)), float(np.float32(high))
    u, u1, u2 = uniforms(a, b)
    if low > -np.inf and high < np.inf:
        return low * (1.0 - u) + high * u                                   # uniform(low, high)
    if low > -np.inf:
        return low - np.log1p(-u)                                           # exponential(1) + low
    if high < np.inf:
        return high - np.log1p(-u)                                          # exponential(1) + high (sic, Box.cs:84)
    return 0.5 + np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)     # normal(0.5, 1) (sic, Box.cs:82)


def one_sided_bound(a, result):
    """Error bound of a one-sided draw -logf(1 - u) + bound in float32: 1 - u is exact, logf is within 4 ulp of ln(1 - u) (the
    OpenCL limit the device math library is built to), the final add rounds once: 4 * spacing(float32(max(|ln(1 - u)|, |result|)))."""
    u = uniforms(a, a)[0]
    big = np.maximum(np.abs(np.log1p(-u)), np.abs(result)).astype(np.float32)
    return 4.0 * np.spacing(big).astype(np.float64)


# Unbounded draw 0.5 + sqrtf(-2 logf(u1)) * cosf(2pi_f32 * u2) in float32: r = sqrt(-2 ln u1) <= sqrt(48 ln 2) = 5.77; the angle
# fl(2pi_f32 * u2) is off by at most 4.2e-7 (half an ulp of 6.28 plus the constant's own 1.7e-7), which moves the cosine by as much;
# cosf adds 4 ulp of a value <= 1 (2.4e-7); logf's 4 ulp at 16.6 are 2.3e-7 relative on r; sqrtf, the two products and the add round
# once each.  Together: 5.77 * (4.2e-7 + 2.4e-7 + 2.3e-7 + 3 * 6e-8) + 2.4e-7 < 6.5e-6, stated as 1e-5 absolute.
UNBOUNDED_BOUND = 1e-5


def wide_bounded_bound(low, high):
    """Bound of the bounded draw for bounds about as wide as float32 (low * (1 - u) + high * u, or low + width * u where the width
    still rounds to a float: products and a sum, each rounded once, every intermediate at most m = max(|low|, |high|)):
    2 * spacing(float32(m)), the spacing taken BELOW m — above float.MaxValue there is none."""
    m = np.float32(max(abs(float(low)), abs(float(high))))
    return 2.0 * (float(m) - float(np.nextafter(m, np.float32(0))))


def discrete_sample(a, n, start):
    """Discrete.Sample() (Discrete.cs:27): start + randint(0, n) = start + ((word A * n) >> 32), in uint64 integers."""
    return (int(start) + ((np.asarray(a, dtype=np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)).astype(np.int32)


def discrete_sample_masked(a, mask, n, start):
    """Discrete.Sample(mask) (Discrete.cs:18-26).  mask: uint8 [count, stride >= n] (one row per lane; columns past n are padding) or
    [n] (one shared row).  valid = {k : mask[k] == 1}; empty -> start, else start + valid[(word A * |valid|) >> 32]."""
    mask = np.asarray(mask, dtype=np.uint8)
    out = np.empty(len(a), dtype=np.int32)
    for i, w in enumerate(a):
        row = mask if mask.ndim == 1 else mask[i]
        valid = [k for k in range(n) if row[k] == 1]
        out[i] = start + (valid[(int(w) * len(valid)) >> 32] if valid else 0)
    return out


def compose_discrete(a, b, n, epsilon, policy):
    """The epsilon-greedy composer (TrainingPlaySession.cs:46-52): explore iff (word B >> 8) / 2^24 <= epsilon (the float32 the ABI
    carries); an exploring lane takes the Discrete.Sample() draw (start 0), every other lane its policy action."""
    explore = uniforms(a, b)[2] <= float(np.float32(epsilon))
    return np.where(explore, discrete_sample(a, n, 0), np.asarray(policy, dtype=np.int32)).astype(np.int32)
