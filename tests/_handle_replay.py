"""A handle's semantics on the CPU (helper module, not a conftest).

Replay is the per-step replay of tests/test_gpu_instantiation_matrix.py: the oracle's step and reset draws, the episode bookkeeping in
NumPy.  HandleModel stands on it and carries EVERYTHING a handle holds between launches — state, observation, reward / done byte of the
last step, the engine tick, the seed and optional per-lane keys, steps_beyond_done, the running and finished episode arrays, terminal
observations — with one method per operation of the public API, each with the engine-tick rule of include/gymnet_amd.h:

  a step or a reset launch is one tick; a decision of R sub-steps is R ticks; ResetWhere(None) on an auto-reset handle is a no-op that
  moves no tick; Seed(int) and Seed(int[]) rewind the tick to 0, SetArray(lane_seeds) installs keys without rewinding it; an all-equal
  key vector is Seed(int); Restore = Seed(int), the arrays, SetState, Tick.

Physics and reset draws come only from the oracle (env_step, env_reset, cartpole_step(kernel_sincos=True), cartpole_reset_f64,
discrete_sample, compose_discrete, box_uniform_sample, sincos_kernel for the observation SetState derives) and from
tests/_action_repeat_model.py for a held decision.  The model never reads a handle.

CONFIGS are the handle configurations tests/test_gpu_call_sequences.py opens; accepted() is the hand-written table of the operations
each of them takes (from the header's and rollout_plan.hpp's documented refusals); apply() runs one operation of
tests/_call_sequences.py on a model."""
import copy

import numpy as np

import _action_repeat_model as ARM
import _instantiation_matrix as M

SEED = 0x5EED
KEYS = np.array([0x1234567, 0x9ABCDEF0123, 77], dtype=np.uint64)     # per-lane Philox keys: lane i gets KEYS[i % 3]


def _lane_seeds(n):
    return KEYS[np.arange(n) % 3]


# ---- the replay ------------------------------------------------------------------------------------------------------------
class Replay:
    """The handle's semantics on the CPU: the oracle's step and reset draws, the episode bookkeeping in NumPy."""

    def __init__(self, oracle, r, s0, sbd0=None, ln0=None, ret0=None):
        self.o, self.r, self.n = oracle, r, r["n"]
        self.f64, self.alias = r["f64"], M.ENVS[r["env"]]["alias"]
        self.s = s0.astype(np.float64 if self.f64 else np.float32)
        self.seeds = _lane_seeds(self.n) if r["lane_seeds"] else None
        self.sbd = None if (r["auto_reset"] or r["env"] not in ("CartPole", "CartPole64")) else np.ascontiguousarray(sbd0, dtype=np.int32)
        self.stats, self.limit = r["episode_stats"], r["max_episode_steps"]
        self.ln = np.zeros(self.n, np.int32) if ln0 is None else ln0.astype(np.int32)
        self.ret = np.zeros(self.n, np.float32) if ret0 is None else ret0.astype(np.float32)
        self.fin_ret, self.fin_len = np.zeros(self.n, np.float32), np.zeros(self.n, np.int32)
        O = 4 if r["env"].startswith("CartPole") else {"Pendulum": 3, "MountainCar": 2, "Acrobot": 6}[r["env"]]
        self.final = np.zeros((O, self.n), self.s.dtype)

    def fresh(self, tick):
        r, n, lo = self.r, self.n, self.r["lane_offset"]
        if self.f64:
            s = self.o.cartpole_reset_f64(SEED, lo, tick, n, lane_seed=self.seeds)
            return s, s
        if self.seeds is None:
            return self.o.env_reset(r["gym"], SEED, lo, tick, n, with_obs=True)
        s, o = self.o.env_reset(r["gym"], int(KEYS[0]), lo, tick, n, with_obs=True)
        for j in (1, 2):
            sj, oj = self.o.env_reset(r["gym"], int(KEYS[j]), lo, tick, n, with_obs=True)
            m = np.arange(n) % 3 == j
            s[:, m], o[:, m] = sj[:, m], oj[:, m]
        return s, o

    def step(self, a, tick):
        """One vector step at engine tick `tick`: returns (obs [O, n], reward, done byte, finished mask)."""
        if self.f64:
            stepped, rw, d, b = self.o.cartpole_step(self.s, a, sbd=self.sbd, dtype=np.float64, kernel_sincos=True)
            if self.sbd is not None:
                self.sbd = b
            obs = stepped
        else:
            stepped, obs, rw, d = self.o.env_step(self.r["gym"], self.s, a, sbd=self.sbd, dtype=np.float32)
        rw = rw.astype(np.float32)
        db = d.astype(np.uint8)
        if self.stats:
            self.ret += rw
            self.ln += 1
            if self.limit:
                db |= np.where(self.ln >= self.limit, 2, 0).astype(np.uint8)
        fin = db != 0
        if self.r["final_obs"]:
            self.final[:, fin] = (stepped if self.alias else obs)[:, fin]
        if self.stats:
            self.fin_ret[fin], self.fin_len[fin] = self.ret[fin], self.ln[fin]
            if self.r["auto_reset"]:
                self.ret[fin], self.ln[fin] = 0.0, 0
        if self.r["auto_reset"] and fin.any():
            fs, fo = self.fresh(tick)
            stepped = np.where(fin, fs, stepped)
            obs = np.where(fin, fo, obs)
        self.s = stepped
        return obs, rw, db, fin


# ---- the configurations ----------------------------------------------------------------------------------------------------
def _cfg(env, n, **flags):
    c = dict(env=env, gym=M.ENVS[env]["gym"], f64=M.ENVS[env]["f64"], n=n, auto_reset=False, done_list=False, episode_stats=False,
             final_obs=False, max_episode_steps=0, double_buffer=False, lane_offset=0, resident=False, lane_seeds=False, launch=None,
             wide=0, share=0.3)
    c.update(flags)
    return c


# 1027 = one full 1024-lane workgroup of the four-lane form and a guarded tail of 3; 4099 = the same beyond the host-mapped small-batch
# path (4096 lanes), so the host boundary stages its copies.  launch: the policy the handle is opened with (the table below has to know
# the lane width to say which action strides a rollout takes); wide: the env's wide lane width (0: the policy's vec is left alone)
CONFIGS = {
    "A": _cfg("CartPole", 1027, auto_reset=True, launch=dict(vec=4, reset_form=1), wide=4),
    "B": _cfg("CartPole", 4099, auto_reset=True, double_buffer=True, done_list=True, episode_stats=True, final_obs=True,
              max_episode_steps=9, lane_offset=(1 << 32) + 5, launch=dict(vec=4), wide=4),
    "C": _cfg("CartPole", 1027, episode_stats=True, launch=dict(vec=1), wide=4),
    "D": _cfg("CartPole64", 1027, auto_reset=True, double_buffer=True, done_list=True, episode_stats=True, launch=dict(vec=2), wide=2),
    "E": _cfg("Pendulum", 1027, auto_reset=True, double_buffer=True, episode_stats=True, max_episode_steps=7, launch=dict(vec=4), wide=4),
    "F": _cfg("Acrobot", 515, done_list=True, episode_stats=True, launch=dict(vec=1)),
    "G": _cfg("CartPole", 7, auto_reset=True, episode_stats=True, resident=True, share=0.6),
}

STEP_LIKE = ("step", "rollout", "rollout_sampled", "rollout_eps", "decision")
# every operation kind of tests/_call_sequences.py
KINDS = STEP_LIKE + ("reset", "reset_where", "seed", "set_lane_seeds", "set_tick", "set_state", "set_array", "set_sbd", "checkpoint",
                     "restore", "migrate", "noop", "refused")
PATHS = {
    "step": ("Step", "StepInt", "StepInto", "StepAsync", "StepDevice"),
    "rollout": ("eager", "graph", "fused"),
    "decision": ("StepRepeat", "StepRepeatDevice"),
    "reset": ("Reset", "ResetDevice"),
    "reset_where": ("ResetWhere", "ResetWhereDevice"),
}


def accepted(c):
    """The operation kinds configuration c takes.  Written by hand from include/gymnet_amd.h and rollout_plan.hpp: epsilon-greedy
    composition is defined for Discrete action spaces; steps_beyond_done exists for CartPole without auto-reset; the episode arrays need
    GYMNET_FLAG_EPISODE_STATS.  A resident handle takes every call (whatever its kernel does not serve makes it leave first), and so does
    a handle with per-lane keys (the fused rollout keys its reset draws with them)."""
    out = set(KINDS)
    if M.ENVS[c["env"]]["box"]:
        out.discard("rollout_eps")
    if c["auto_reset"] or not c["env"].startswith("CartPole"):
        out.discard("set_sbd")
    if not c["episode_stats"]:
        out.discard("set_array")
    return out


def refusals(c):
    """The calls configuration c must refuse: the generic ones, and the kinds accepted() leaves out."""
    out = ["bad_policy", "ring0", "repeat256", "epsilon", "restore_num_envs"]
    if c["wide"]:
        out.append("misaligned")                  # (only while the policy's vec is the wide one: the sequence knows)
    if not M.ENVS[c["env"]]["alias"]:
        out.append("reset_form1")                 # the wave-compacted reset belongs to the envs whose observation is the state
    acc = accepted(c)
    out += [k for k in ("set_sbd", "set_array") if k not in acc]
    return out


def obs_dim(c):
    return 4 if c["env"].startswith("CartPole") else {"Pendulum": 3, "Acrobot": 6}[c["env"]]


def state_dim(c):
    return 2 if c["env"] == "Pendulum" else 4


# ---- the model --------------------------------------------------------------------------------------------------------------
class HandleModel(Replay):
    """Everything a handle of configuration c holds between launches, from gymnet_vecenv_create on (zero state, tick 0)."""

    def __init__(self, oracle, c, seed=SEED, n=None, lane_offset=None):
        c = dict(c, lane_seeds=False)
        if n is not None:
            c["n"] = n
        if lane_offset is not None:
            c["lane_offset"] = lane_offset
        super().__init__(oracle, c, np.zeros((state_dim(c), c["n"])), sbd0=np.full(c["n"], -1, np.int32))
        self.c, self.lo = c, c["lane_offset"]
        self.dtype = self.s.dtype
        self.seed, self.tick = int(seed) & 0xFFFFFFFFFFFFFFFF, 0
        self.obs = np.zeros((obs_dim(c), self.n), self.dtype)
        self.reward, self.done = np.zeros(self.n, np.float32), np.zeros(self.n, np.uint8)
        self.lane_steps = 0
        self.last_fin = None                    # lanes the last step-like operation finished (the done list describes them)
        self.draw_ticks = []                    # the ticks reset draws were made at, in order (the host test's coverage conditions)

    # -- draws -----------------------------------------------------------------------------------------------------------------
    def _draw(self, key, tick):
        if self.f64:
            s = self.o.cartpole_reset_f64(key, self.lo, tick, self.n)
            return s, s.copy()
        return self.o.env_reset(self.r["gym"], key, self.lo, tick, self.n, with_obs=True)

    def _keys(self):
        return [(self.seed, np.ones(self.n, bool))] if self.seeds is None else [(int(k), self.seeds == k) for k in np.unique(self.seeds)]

    def fresh(self, tick):
        self.draw_ticks.append(int(tick))
        s = o = None
        for key, m in self._keys():
            sk, ok = self._draw(key, tick)
            if s is None:
                s, o = sk.copy(), ok.copy()
            else:
                s[:, m], o[:, m] = sk[:, m], ok[:, m]
        return s, o

    def observe(self, s):
        """The observation SetState derives from a state (envs.hpp observe): the step's own sin / cos"""
        s = np.asarray(s, self.dtype)
        if self.alias:
            return s.copy()
        if self.r["env"] == "Pendulum":
            sn, cs = self.o.sincos_kernel(s[0])
            return np.stack([cs, sn, s[1]]).astype(self.dtype)
        assert np.abs(s[:2]).max() < 24.0          # Acrobot: the small-argument form the step itself takes
        s1, c1 = self.o.sincos_kernel(s[0], small=True)
        s2, c2 = self.o.sincos_kernel(s[1], small=True)
        return np.stack([c1, s1, c2, s2, s[2], s[3]]).astype(self.dtype)

    def _act(self, a):
        box = M.ENVS[self.r["env"]]["box"]
        a = np.asarray(a)
        if a.ndim == 0:                            # IVecEnv.Step(int): one scalar for every lane (on a Box space: the torque)
            a = np.full(self.n, a)
        return np.ascontiguousarray(a.astype(np.float32 if box else np.int32))

    # -- step-like ---------------------------------------------------------------------------------------------------------------
    def step(self, a):
        a = self._act(a)
        obs, rw, db, fin = Replay.step(self, a, self.tick)
        self.s = np.array(self.s, self.dtype)
        self.obs, self.reward, self.done = np.array(obs, self.dtype), rw, db
        self.tick += 1
        self.lane_steps += self.n
        self.last_fin = fin
        rec = dict(a=a, obs=self.obs.copy(), reward=rw.copy(), done=db.copy(), lanes=np.nonzero(fin)[0],
                   fin_ret=self.fin_ret[fin].copy(), fin_len=self.fin_len[fin].copy())
        return rec

    def rollout(self, ring, T):
        ring = np.asarray(ring)
        return [self.step(ring[t % len(ring)]) for t in range(T)]

    def sampled_action(self, aseed, atick):
        e = M.ENVS[self.r["env"]]
        if e["box"]:
            return self.o.box_uniform_sample(aseed, self.lo, atick, -2.0, 2.0, self.n)
        return self.o.discrete_sample(aseed, self.lo, atick, e["nvals"], 0, self.n)

    def rollout_sampled(self, T, aseed, atick0):
        return [self.step(self.sampled_action(aseed, atick0 + t)) for t in range(T)]

    def rollout_eps(self, T, eps, ring, aseed, atick0):
        nv = M.ENVS[self.r["env"]]["nvals"]
        ring = np.asarray(ring, np.int32)
        return [self.step(self.o.compose_discrete(aseed, self.lo, atick0 + t, nv, eps, ring[t % len(ring)])) for t in range(T)]

    def decision(self, a, R):
        """`a` held for R sub-steps in one launch (tests/_action_repeat_model.py; lanes are independent, so with per-lane keys the
        decision is replayed once per key and every lane takes the replay of its own)."""
        a = self._act(a)
        name = "CartPole64" if self.f64 else self.r["env"]
        merged = None
        for key, m in self._keys():
            rm = ARM.RepeatModel(name, self.s, key, self.lo, self.r["auto_reset"], self.stats, self.limit, sbd0=self.sbd, ret0=self.ret, len0=self.ln)
            rm.fin_ret, rm.fin_len = self.fin_ret.copy(), self.fin_len.copy()
            out = rm.decision(a, R, self.tick)
            if out["final_obs"] is None:
                out["final_obs"] = np.zeros_like(out["obs"])
            if merged is None:
                merged = out
            else:
                for k, v in out.items():
                    if v is not None:
                        merged[k][..., m] = v[..., m]
        out = merged
        fin = out["finished_at"] >= 0
        self.s, self.obs = out["state"].astype(self.dtype), out["obs"].astype(self.dtype)
        if self.sbd is not None:
            self.sbd = out["sbd"]
        self.reward, self.done = out["reward"], out["done"]
        if self.stats:
            self.ret, self.ln, self.fin_ret, self.fin_len = out["ep_ret"], out["ep_len"], out["fin_ret"], out["fin_len"]
        if self.r["final_obs"]:
            self.final[:, fin] = out["final_obs"][:, fin]
        if self.r["auto_reset"]:
            self.draw_ticks += sorted({self.tick + int(r) for r in out["finished_at"][fin]})
        self.tick += R
        self.lane_steps += R * self.n
        self.last_fin = fin
        return dict(a=a, obs=self.obs.copy(), reward=self.reward.copy(), done=self.done.copy(), lanes=np.nonzero(fin)[0])

    # -- resets ------------------------------------------------------------------------------------------------------------------
    def reset_where(self, mask):
        if mask is None:
            if self.r["auto_reset"]:
                return                              # the step already re-drew every finished lane: a no-op that moves no tick
            mask = self.done != 0
        m = np.asarray(mask).astype(bool)
        fs, fo = self.fresh(self.tick)
        self.s[:, m], self.obs[:, m] = fs[:, m], fo[:, m]
        if self.sbd is not None:
            self.sbd[m] = -1
        self.done[m] = 0
        if self.stats:
            self.ret[m], self.ln[m] = 0.0, 0
        self.tick += 1

    def reset(self):
        self.reset_where(np.ones(self.n, bool))

    # -- mutators ----------------------------------------------------------------------------------------------------------------
    def seed_with(self, value):
        if np.ndim(value) == 0:
            self.seed, self.seeds = int(value) & 0xFFFFFFFFFFFFFFFF, None
        else:
            keys = np.asarray(value, np.int64).astype(np.uint64)
            if (keys == keys[0]).all():              # VecEnv.Seed(int) reaches the lanes as N equal seeds
                self.seed, self.seeds = int(keys[0]), None
            else:
                self.seeds = keys.copy()
        self.tick = 0

    def set_lane_seeds(self, keys):
        self.seeds = np.asarray(keys, np.int64).astype(np.uint64)          # (the tick stays)

    def set_tick(self, v):
        self.tick = int(v)

    def set_state(self, s):
        self.s = np.array(s, self.dtype)
        self.obs = self.observe(self.s)

    def set_array(self, name, v):
        if name == "episode_length":
            self.ln = np.array(v, np.int32)
        else:
            self.ret = np.array(v, np.float32)

    def set_sbd(self, v):
        self.sbd = np.array(v, np.int32)

    _CK = ("s", "reward", "done", "sbd", "ret", "ln", "fin_ret", "fin_len", "final", "seeds", "seed", "tick")

    def checkpoint(self):
        return {k: copy.deepcopy(getattr(self, k)) for k in self._CK}

    def restore(self, ck):
        for k in self._CK:
            setattr(self, k, copy.deepcopy(ck[k]))
        self.obs = self.observe(self.s)             # Restore hands the state to SetState
        self.last_fin = None

    def migrated(self):
        """The handle was replaced by a fresh one that restored its checkpoint: the counters start again."""
        self.lane_steps = 0
        self.last_fin = None

    def snapshot(self):
        return {k: copy.deepcopy(getattr(self, k)) for k in self._CK + ("obs", "lane_steps")}


def apply(model, op, slots):
    """One operation of tests/_call_sequences.py on the model.  slots: the model's checkpoints by name.  Returns what the operation
    recorded (a step record, a list of them, or None)."""
    k = op["kind"]
    if k == "step":
        return model.step(op["a"])
    if k == "rollout":
        return model.rollout(op["ring"], op["T"])
    if k == "rollout_sampled":
        return model.rollout_sampled(op["T"], op["aseed"], op["atick0"])
    if k == "rollout_eps":
        return model.rollout_eps(op["T"], op["eps"], op["ring"], op["aseed"], op["atick0"])
    if k == "decision":
        return model.decision(op["a"], op["R"])
    if k == "reset":
        return model.reset()
    if k == "reset_where":
        return model.reset_where(op["mask"])
    if k == "seed":
        return model.seed_with(op["value"])
    if k == "set_lane_seeds":
        return model.set_lane_seeds(op["value"])
    if k == "set_tick":
        return model.set_tick(op["value"])
    if k == "set_state":
        return model.set_state(op["state"])
    if k == "set_array":
        return model.set_array(op["name"], op["value"])
    if k == "set_sbd":
        return model.set_sbd(op["value"])
    if k == "checkpoint":
        slots[op["slot"]] = model.checkpoint()
        return None
    if k == "restore":
        return model.restore(slots[op["slot"]])
    if k == "migrate":
        return model.migrated()
    assert k in ("noop", "refused"), k
    return None


def _bits(a):
    """integer views of floating arrays: -0.0 is not +0.0; every NaN counts as one value"""
    if a.dtype.kind != "f":
        return a
    v = np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).copy()
    v[np.isnan(a)] = ~v.dtype.type(0)
    return v


def first_diff(a, b):
    """None where a and b are equal bit for bit (NaN equal to NaN), else (index, a's element, b's) of the first difference"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return ("shape", a.shape, b.shape)
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        if a.dtype != b.dtype:
            return ("dtype", a.dtype, b.dtype)
    d = np.argwhere(_bits(a) != _bits(b))
    return None if len(d) == 0 else (tuple(int(x) for x in d[0]), a[tuple(d[0])], b[tuple(d[0])])
