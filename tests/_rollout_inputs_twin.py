"""gymnet_rollout_inputs_device restated in NumPy (include/gymnet_amd.h): the push rule applied T times to a [S, O, n] history, on uint32
bit patterns so that nothing a value passes through can change it.  It does not look back over done bytes the way the kernels of
gym.net_amd/csrc/rollout_inputs.hip do: it is an independent statement of the same contract.  Also the inputs the tests share: shapes,
done patterns, observations as random bits with the special values planted, and float64 observations with the rounding cases."""
import numpy as np

U32 = np.uint32
NAN_BITS = 0x7FC00000

# (obs_dim, history): the envs' own (CartPole 4, Acrobot 6, Pendulum 3), one slot, and the widest inputs an actor can have
SHAPES = ((4, 4), (4, 1), (6, 4), (3, 21), (2, 32), (1, 64), (4, 16))
COUNTS = (1, 3, 67, 256, 1028)               # a single lane, a partial wave, a ragged block, whole blocks, a second block's tail
PATTERNS = ("none", "ones", "both_bits", "first_row", "last_row", "runs", "bernoulli")


def steps_for(S):
    """T in {1, 2, S-1, S, S+1, 37}: around the look-back of S - 1 rows, and longer than the rows kept in flight"""
    return tuple(sorted({T for T in (1, 2, S - 1, S, S + 1, 37) if T >= 1}))


def f32_bits(a):
    """float32 bit patterns of a float32 or float64 array (float64: rounded to nearest even, beyond the range to inf)"""
    a = np.asarray(a)
    if a.dtype == np.float64:
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            a = a.astype(np.float32)
    assert a.dtype == np.float32, a.dtype
    return np.ascontiguousarray(a).view(U32)


def inputs(rec_obs, rec_done, history0):
    """rec_obs [T, O, n] float32 / float64, rec_done uint8 [T, n], history0 float32 [S, O, n] -> (x uint32 [T, n, S * O], the history
    after the last step uint32 [S, O, n])"""
    H = f32_bits(history0).copy()
    S, O, n = H.shape
    T = rec_obs.shape[0]
    obs = f32_bits(rec_obs).reshape(T, O, n)
    x = np.empty((T, n, S * O), U32)
    for t in range(T):
        x[t] = H.transpose(2, 0, 1).reshape(n, S * O)                      # the input of step t
        o, d = obs[t], np.asarray(rec_done[t]) != 0
        pushed = np.concatenate([H[1:], o[None]], axis=0)                  # H[s] = H[s + 1], the last row = o
        refilled = np.broadcast_to(o[None], H.shape)                       # every row = o
        H = np.where(d[None, None, :], refilled, pushed)
    return x, H


def gathered(x, rows):
    """dense x uint32 [T, n, W] and flat row indices -> [m, W]; an index outside [0, T * n) gives canonical NaNs"""
    flat = x.reshape(-1, x.shape[-1])
    rows = np.asarray(rows, np.int64)
    ok = (rows >= 0) & (rows < flat.shape[0])
    out = np.full((len(rows), x.shape[-1]), NAN_BITS, U32)
    out[ok] = flat[rows[ok]]
    return out


def done_pattern(name, T, n, S, rng):
    d = np.zeros((T, n), np.uint8)
    if name == "ones":
        d[:] = 1
    elif name == "both_bits":                                              # every done value, on a third of the elements
        d[:] = rng.integers(1, 4, (T, n)) * (rng.random((T, n)) < 1.0 / 3.0)
        d.reshape(-1)[:3] = (1, 2, 3)[:min(3, d.size)]
    elif name == "first_row":
        d[0] = 2
    elif name == "last_row":
        d[T - 1] = 1
    elif name == "runs":                                                   # runs of 1 .. 3 consecutive dones, a gap of 0 .. S rows between them
        for i in range(n):
            t = int(rng.integers(0, S + 1))
            while t < T:
                run = int(rng.integers(1, 4))
                d[t:t + run, i] = rng.integers(1, 4, len(d[t:t + run, i]))
                t += run + int(rng.integers(0, S + 1))
    elif name == "bernoulli":
        d[:] = (rng.random((T, n)) < 1.0 / S) * rng.integers(1, 4, (T, n))
    else:
        assert name == "none", name
    return d


SPECIAL_BITS = (0x80000000, 0x00000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FA00001, 0xFFC12345, 0x7F800001)
# -0.0, +0.0, the smallest denormal, the largest negative denormal, +-inf, the canonical NaN, a signalling NaN, NaNs with payloads


def random_bits(shape, rng):
    """float32 values as random bit patterns (NaN payloads, denormals and infinities among them) with SPECIAL_BITS planted up front"""
    a = rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(U32)
    flat = a.reshape(-1)
    k = min(len(SPECIAL_BITS), flat.size)
    flat[:k] = SPECIAL_BITS[:k]
    return a.view(np.float32)


F64_SPECIALS = (
    1.0 + 2.0 ** -24,                # half-way between 1 and its float32 successor: to even, 1.0
    1.0 + 3.0 * 2.0 ** -24,          # half-way, the other parity: up
    -(1.0 + 2.0 ** -24), 1.0 + 2.0 ** -24 + 2.0 ** -52, 1.0 + 2.0 ** -24 - 2.0 ** -52,       # a bit to either side of a half-way point
    3.4028235677973366e38,           # FLT_MAX plus half a spacing: to even, inf
    3.4028235677973362e38,           # just below it: FLT_MAX
    1e39, -1e39, 1.7976931348623157e308,                                   # beyond the range: +-inf
    5e-324, -5e-324, 2.2250738585072014e-308, 1e-310,                      # float64 denormals and the smallest normal: +-0
    1e-40, -1e-40, 2.0 ** -149, 2.0 ** -150, 3.0 * 2.0 ** -150, 2.0 ** -150 + 2.0 ** -200, 2.0 ** -126 - 2.0 ** -150,   # float32 denormal results, with ties
    0.0, -0.0, np.inf, -np.inf,
)


def random_f64(shape, rng):
    a = rng.standard_normal(shape) * np.exp(rng.uniform(-3, 3, shape))
    flat = a.reshape(-1)
    k = min(len(F64_SPECIALS), flat.size)
    flat[:k] = F64_SPECIALS[:k]
    return a


_cases = {}


def case(O, S, T, n, pattern, seed=0, f64=False):
    """the shared inputs of one case and the twin's outputs, computed once: a dict of rec_obs [T, O, n], rec_done [T, n], history0 [S, O, n],
    x uint32 [T, n, S * O], history_out uint32 [S, O, n]"""
    key = (O, S, T, n, pattern, seed, f64)
    if key not in _cases:
        rng = np.random.default_rng([O, S, T, n, PATTERNS.index(pattern), seed, int(f64)])
        c = {"rec_obs": random_f64((T, O, n), rng) if f64 else random_bits((T, O, n), rng),
             "rec_done": done_pattern(pattern, T, n, S, rng), "history0": random_bits((S, O, n), rng)}
        c["x"], c["history_out"] = inputs(c["rec_obs"], c["rec_done"], c["history0"])
        for v in c.values():
            v.setflags(write=False)
        _cases[key] = c
    return _cases[key]
