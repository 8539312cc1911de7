"""CPU twins of MountainCarContinuous-v0 (helper module, not a conftest).

Two NumPy restatements of upstream gym's continuous_mountain_car.py step (the env is absent from the reference):
  step_f64 — the upstream algorithm in float64: what the golden fixture (tests/golden/mountaincar_continuous.npz) is made from;
  step_f32 — the kernel's semantics (csrc/envs.hpp MountainCarContinuous::step): its operation order in np.float32, every operation
             rounded on its own (the kernels are built with -ffp-contract=off), cos from oracle.sincos_kernel — the CPU restatement of
             cos_f32, bit-identical to it for |3 p| <= 65536.  The GPU must equal it BIT FOR BIT.
Resets are MountainCar's draw (the kernel calls MountainCar::reset): oracle.mountaincar_reset, per Philox key.  In-kernel actions are
Box(-1, 1).Sample(): oracle.box_uniform_sample(seed, lane0, tick, -1, 1, n).  Replay keeps the episode bookkeeping in NumPy."""
import numpy as np

F32 = np.float32
GOAL_BITS = 0x3EE66667                                   # smallest float32 >= 0.45 (0.45f = 0x3EE66666 lies below 0.45)
GOAL32 = np.array([GOAL_BITS], np.uint32).view(np.float32)[0]
BELOW_GOAL32 = np.array([GOAL_BITS - 1], np.uint32).view(np.float32)[0]
ACTION_LOW, ACTION_HIGH = -1.0, 1.0
GYM = "MountainCarContinuous-v0"


def _oracle():
    from oracle import capi
    return capi


def kcos(x):
    """cos_f32 of the kernel (envs.hpp), restated on the CPU by the oracle."""
    return _oracle().sincos_kernel(np.asarray(x, F32))[1]


def step_f64(state, action):
    """Upstream step in float64 over SoA state [2, n]: returns (state [2, n] f64, reward f64 [n], done bool [n])."""
    p = np.array(state[0], np.float64)
    v = np.array(state[1], np.float64)
    a = np.asarray(action, np.float64).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        force = np.minimum(np.maximum(a, -1.0), 1.0)                      # min(max(action[0], min_action), max_action)
        v = v + (force * 0.0015 - 0.0025 * np.cos(3 * p))                 # velocity += force * power - 0.0025 * cos(3 * position)
        v = np.where(v > 0.07, 0.07, v)
        v = np.where(v < -0.07, -0.07, v)
        p = p + v
        p = np.where(p > 0.6, 0.6, p)
        p = np.where(p < -1.2, -1.2, p)
        v = np.where((p == -1.2) & (v < 0), 0.0, v)
        done = (p >= 0.45) & (v >= 0.0)
        reward = np.where(done, 100.0, 0.0) - a ** 2 * 0.1                # reward -= math.pow(action[0], 2) * 0.1: the RAW action
    return np.stack([p, v]), reward, done


def step_f32(state, action):
    """The kernel's step, operation for operation in float32: returns (state [2, n] f32, reward f32 [n], done bool [n])."""
    p = np.array(state[0], F32)
    v = np.array(state[1], F32)
    a = np.asarray(action, F32).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        force = np.where(a < F32(-1), F32(-1), np.where(a > F32(1), F32(1), a))   # NaN and -0.0 pass through
        c = kcos(F32(3) * p)
        v = v + (force * F32(0.0015) - F32(0.0025) * c)
        v = np.where(v < F32(-0.07), F32(-0.07), np.where(v > F32(0.07), F32(0.07), v))
        p = p + v
        p = np.where(p < F32(-1.2), F32(-1.2), np.where(p > F32(0.6), F32(0.6), p))
        v = np.where((p == F32(-1.2)) & (v < F32(0)), F32(0), v)
        done = (p >= GOAL32) & (v >= F32(0))
        reward = np.where(done, F32(100), F32(0)) - (a * a) * F32(0.1)
    return np.stack([p, v]).astype(F32), reward.astype(F32), done


def reset(seed, lane0, tick, n, lane_seeds=None):
    """The fused / explicit reset draw of lanes lane0 .. lane0 + n - 1 at `tick`: MountainCar's, keyed by `seed` or by lane_seeds[i]."""
    o = _oracle()
    if lane_seeds is None:
        return o.mountaincar_reset(int(seed), int(lane0), int(tick), n)
    lane_seeds = np.asarray(lane_seeds, np.uint64)
    s = np.zeros((2, n), F32)
    for key in np.unique(lane_seeds):
        m = lane_seeds == key
        s[:, m] = o.mountaincar_reset(int(key), int(lane0), int(tick), n)[:, m]
    return s


def box_sample(seed, lane0, tick, n):
    """ActionSpace.Sample() drawn in the kernel for (seed, global lanes lane0.., tick)."""
    return _oracle().box_uniform_sample(int(seed), int(lane0), int(tick), ACTION_LOW, ACTION_HIGH, n)


class Replay:
    """A handle's semantics on the CPU: step_f32, the fused reset, the episode bookkeeping (time limit = done bit 1)."""

    def __init__(self, s0, seed, lane_offset, auto_reset, episode_stats=False, max_episode_steps=0, final_obs=False, lane_seeds=None,
                 ln0=None, ret0=None):
        self.s = np.array(s0, F32)
        self.n = self.s.shape[1]
        self.seed, self.lo, self.auto = seed, lane_offset, auto_reset
        self.stats, self.limit, self.keep_final = episode_stats, max_episode_steps, final_obs
        self.lane_seeds = lane_seeds
        self.ln = np.zeros(self.n, np.int32) if ln0 is None else np.array(ln0, np.int32)
        self.ret = np.zeros(self.n, F32) if ret0 is None else np.array(ret0, F32)
        self.fin_ret, self.fin_len = np.zeros(self.n, F32), np.zeros(self.n, np.int32)
        self.final = np.zeros((2, self.n), F32)

    def step(self, a, tick):
        """One vector step at engine tick `tick`: returns (obs [2, n], reward, done byte, finished mask)."""
        s, rw, d = step_f32(self.s, a)
        db = d.astype(np.uint8)
        if self.stats:
            self.ret = (self.ret + rw).astype(F32)
            self.ln += 1
            if self.limit:
                db |= np.where(self.ln >= self.limit, 2, 0).astype(np.uint8)
        fin = db != 0
        if self.keep_final:
            self.final[:, fin] = s[:, fin]
        if self.stats:
            self.fin_ret[fin], self.fin_len[fin] = self.ret[fin], self.ln[fin]
            if self.auto:
                self.ret[fin], self.ln[fin] = 0.0, 0
        if self.auto and fin.any():
            s = np.where(fin, reset(self.seed, self.lo, tick, self.n, self.lane_seeds), s)
        self.s = s
        return s.copy(), rw, db, fin
