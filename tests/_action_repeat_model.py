"""Frame skip in NumPy, one decision at a time (helper module, not a conftest): the semantics of gymnet_vecenv_step_repeat_device
(include/gymnet_amd.h) built on the per-step functions the GPU suite already replays with — oracle.env_step / oracle.env_reset in the
handle's dtype, oracle.cartpole_step(kernel_sincos=True) / oracle.cartpole_reset_f64 for the float64 engine, and
tests/_mountaincar_continuous_twin.py for MountainCarContinuous.  Every comparison against it is bitwise.

A decision of R sub-steps starting at engine tick tick0: every lane is live at sub-step 0; a live lane takes the one-step kernel's step at
tick tick0 + r (physics, steps_beyond_done rule, episode return / length, time limit); a lane whose done byte comes out non-zero at
sub-step r keeps that byte as the decision's, leaves its finished-episode values, is re-drawn with the reset draw of tick tick0 + r on an
auto-reset handle, and is idle for the rest of the decision.  The decision's reward starts from the first sub-step's reward itself."""
import numpy as np

import _mountaincar_continuous_twin as mcc

F32 = np.float32
CARTPOLE, PENDULUM, MOUNTAINCAR, ACROBOT = "CartPole-v1", "Pendulum-v1", "MountainCar-v0", "Acrobot-v1"
# name -> (gym id, numpy dtype of the state, Box action?, number of discrete actions)
ENVS = {"CartPole": (CARTPOLE, F32, False, 2), "CartPole64": (CARTPOLE, np.float64, False, 2), "Pendulum": (PENDULUM, F32, True, 0),
        "MountainCar": (MOUNTAINCAR, F32, False, 3), "MountainCarContinuous": (mcc.GYM, F32, True, 0), "Acrobot": (ACROBOT, F32, False, 3)}


def _oracle():
    from oracle import capi
    return capi


def step_once(name, state, action, sbd=None):
    """One env step of every lane in the handle's dtype: (state, obs, reward f32, done u8, sbd).  sbd (CartPole without auto-reset):
    the steps_beyond_done rule is applied and the new counters returned; None: the plain step."""
    o = _oracle()
    gym, dt, _, _ = ENVS[name]
    if gym == CARTPOLE:
        s, rw, dn, b = o.cartpole_step(state, action, sbd, dtype=dt, kernel_sincos=(dt == np.float64))
        return s, s.copy(), rw.astype(F32), dn, (b if sbd is not None else None)
    if gym == mcc.GYM:
        s, rw, dn = mcc.step_f32(state, action)
        return s, s.copy(), rw.astype(F32), dn.astype(np.uint8), None
    s, obs, rw, dn = o.env_step(gym, state, action, dtype=F32)
    return s, obs, rw.astype(F32), dn, None


def reset_draw(name, seed, lane0, tick, n):
    """(state, obs) of the reset draw of global lanes lane0 .. lane0 + n - 1 at `tick`"""
    o = _oracle()
    gym, dt, _, _ = ENVS[name]
    if gym == CARTPOLE:
        s = o.cartpole_reset_f64(seed, lane0, tick, n) if dt == np.float64 else o.cartpole_reset(seed, lane0, tick, n)
        return s, s.copy()
    if gym == mcc.GYM:
        s = mcc.reset(seed, lane0, tick, n)
        return s, s.copy()
    return o.env_reset(gym, seed, lane0, tick, n, with_obs=True)


class RepeatModel:
    """A handle's semantics on the CPU.  state0: SoA [S, n] in the handle's dtype; sbd0: steps_beyond_done (CartPole without auto-reset)."""

    def __init__(self, name, state0, seed, lane_offset=0, auto_reset=True, stats=False, limit=0, sbd0=None, ret0=None, len0=None):
        self.name = name
        self.dtype = ENVS[name][1]
        self.s = np.array(state0, self.dtype)
        self.n = self.s.shape[1]
        self.obs = None                      # set by the first decision (the handle's own d_obs is whatever the reset left)
        self.seed, self.lo, self.auto, self.stats, self.limit = int(seed), int(lane_offset), bool(auto_reset), bool(stats), int(limit)
        self.has_sbd = ENVS[name][0] == CARTPOLE and not self.auto
        self.sbd = (np.full(self.n, -1, np.int32) if sbd0 is None else np.array(sbd0, np.int32)) if self.has_sbd else None
        self.ret = np.zeros(self.n, F32) if ret0 is None else np.array(ret0, F32)
        self.len = np.zeros(self.n, np.int32) if len0 is None else np.array(len0, np.int32)
        self.fin_ret, self.fin_len = np.zeros(self.n, F32), np.zeros(self.n, np.int32)
        self.final_obs = None
        self.after_done = 0                  # steps taken on lanes that had already returned done (CartPole without auto-reset)
        self.episodes = 0

    def decision(self, action, R, tick0):
        """One decision: `action` held for R sub-steps from engine tick tick0.  Returns a dict: state, obs, sbd, reward (the float32 sum),
        done (the decision's byte), ep_ret / ep_len (running), fin_ret / fin_len / final_obs (finished-episode views), finished_at
        (per lane: the sub-step at which it finished, -1 = it did not)."""
        n = self.n
        live = np.ones(n, bool)
        reward = np.zeros(n, F32)
        done = np.zeros(n, np.uint8)
        finished_at = np.full(n, -1, np.int32)
        for r in range(R):
            s, obs, rw, dn, sbd = step_once(self.name, self.s, action, self.sbd.copy() if self.has_sbd else None)
            db = dn.astype(np.uint8)
            if self.has_sbd:
                self.after_done += int((live & (dn != 0) & (self.sbd != -1)).sum())
                self.sbd = np.where(live, sbd, self.sbd).astype(np.int32)
            if self.stats:
                ret = (self.ret + rw).astype(F32)
                ln = self.len + 1
                if self.limit > 0:
                    db = db | np.where(ln >= self.limit, 2, 0).astype(np.uint8)
                self.ret = np.where(live, ret, self.ret).astype(F32)
                self.len = np.where(live, ln, self.len).astype(np.int32)
            fin = live & (db != 0)
            self.s = np.where(live, s, self.s).astype(self.dtype)
            self.obs = obs.copy() if self.obs is None else np.where(live, obs, self.obs).astype(self.dtype)
            # the reward starts from the first sub-step's reward ITSELF (a -0.0f survives), then adds in sub-step order
            reward = rw.copy() if r == 0 else np.where(live, (reward + rw).astype(F32), reward).astype(F32)
            done = np.where(fin, db, done).astype(np.uint8)
            finished_at[fin] = r
            if fin.any():
                self.episodes += int(fin.sum())
                if self.final_obs is None:
                    self.final_obs = np.zeros_like(self.obs)
                self.final_obs[:, fin] = self.obs[:, fin]
                if self.stats:
                    self.fin_ret[fin], self.fin_len[fin] = self.ret[fin], self.len[fin]
                    if self.auto:
                        self.ret[fin], self.len[fin] = 0.0, 0
                if self.auto:
                    rs, ro = reset_draw(self.name, self.seed, self.lo, tick0 + r, n)
                    self.s[:, fin] = rs[:, fin]
                    self.obs[:, fin] = ro[:, fin]
            live = live & ~fin
        return {"state": self.s.copy(), "obs": self.obs.copy(), "sbd": None if self.sbd is None else self.sbd.copy(), "reward": reward,
                "done": done, "ep_ret": self.ret.copy(), "ep_len": self.len.copy(), "fin_ret": self.fin_ret.copy(),
                "fin_len": self.fin_len.copy(), "final_obs": None if self.final_obs is None else self.final_obs.copy(),
                "finished_at": finished_at}
