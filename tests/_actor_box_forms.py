"""The recipe table of the fused Box-actor rollout's kernels (helper module, not a conftest), the composition rule of a Box actor in
NumPy, and the comparison every recipe runs.

actor_box.hip compiles actor_box_rollout_kernel<Env, AUTORESET, EXTRAS, RECORDS> in 12 forms: Pendulum and MountainCarContinuous x
auto-reset on / off x {lean, bookkeeping, bookkeeping with episode records}.  Each row of FORMS names one form the way the assembly
demangles it and says how to reach it through the public API, as tests/_actor_forms.py does for the Discrete actor: the env, the
handle's auto_reset and its shape.  tests/test_actor_box_host.py pins the table to the compiled set; tests/test_gpu_actor_box.py runs
every row.

The rule (include/gymnet_amd.h, gymnet_vecenv_actor_box_config): the greedy action is raw < low ? low : (raw > high ? high : raw); a
lane whose word B of the aux stream is <= coin_threshold(epsilon) takes low + (high - low) * u01_24(word A) instead."""
import numpy as np

import _actor_forms as forms

F32 = np.float32
ENVS = {"Pendulum": "Pendulum-v1", "MountainCarContinuous": "MountainCarContinuous-v0"}
BOUNDS = {"Pendulum-v1": (-2.0, 2.0), "MountainCarContinuous-v0": (-1.0, 1.0)}
SHAPES, LIMIT = forms.SHAPES, forms.LIMIT


def _b(v):
    return "true" if v else "false"


FORMS = [dict(kernel=f"actor_box_rollout_kernel<{env},{_b(ar)},{_b(SHAPES[shape][0])},{_b(SHAPES[shape][1])}>", env=gym, auto_reset=ar, shape=shape)
         for env, gym in ENVS.items() for ar in (True, False) for shape in SHAPES]


def form_id(row):
    return row["kernel"]


def coin_threshold(eps):
    """philox.hpp coin_threshold: u01_24(w) <= epsilon exactly when w <= this (epsilon * 2^24 is exact in float32)"""
    t = np.floor(np.float64(F32(eps)) * 16777216.0)
    if not t >= 0:
        return 0
    return 0xFFFFFFFF if t >= 16777215.0 else (int(t) << 8) | 0xFF


def clamp(raw, low, high):
    """the envs' own form: a NaN fails both compares and passes"""
    raw = np.asarray(raw, F32)
    with np.errstate(invalid="ignore"):
        return np.where(raw < F32(low), F32(low), np.where(raw > F32(high), F32(high), raw)).astype(F32)


def u01_24(words):
    return (np.asarray(words, np.uint32) >> np.uint32(8)).astype(F32) * F32(1.0 / 16777216.0)


def sample(words_a, low, high):
    """Box(low, high).Sample() of the bounded regime, every operation rounded to float32 on its own"""
    return (F32(low) + (F32(high) - F32(low)) * u01_24(words_a)).astype(F32)


def compose(raw, words_a, words_b, eps, low, high):
    """(actions float32, explore bool) of one act call from the unclamped outputs and the lanes' words A and B"""
    explore = np.asarray(words_b, np.uint32) <= np.uint32(coin_threshold(eps))
    return np.where(explore, sample(words_a, low, high), clamp(raw, low, high)).astype(F32), explore


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def fused_equals_single_steps(gpu_pkg, name, n, T, kw, records_on, pairs, S=4, eps=0.3, seed=99, tick0=1000, prepare=None, env_seed=0xAC7,
                              warm=0, after_warm=None, lane_offset=0):
    """_actor_forms.fused_equals_single_steps for a Box actor: handle a runs T x actor.Step (Act, StepDevice, Push), its twin b one fused
    rollout with actions="actor", and the recorded actions (float32 bit patterns), observations, rewards and dones, the state, done
    bytes, tick, history, episode statistics, the episode records as sets, count[1] and, without auto-reset, the stepped-after-done
    counter are equal; both accept the next single step.  prepare(env) runs on each handle after Reset and before its actor is
    configured; warm closed-loop single steps come first on both, then after_warm(env, actor).  Returns what handle a saw."""
    import torch
    host = forms.host
    bookkeeping = bool(kw.get("episode_stats"))
    assert not records_on or bookkeeping
    with gpu_pkg.VectorEnv(name, n, seed=env_seed, lane_offset=lane_offset, **kw) as a, \
            gpu_pkg.VectorEnv(name, n, seed=env_seed, lane_offset=lane_offset, **kw) as b:
        a.Reset(); b.Reset()
        if prepare:
            prepare(a); prepare(b)
        O = a.ObsDim
        actor_a, actor_b = a.Actor(pairs, S), b.Actor(pairs, S)
        for t in range(warm):
            actor_a.Step(eps, seed + 1, t); actor_b.Step(eps, seed + 1, t)
        if after_warm:
            after_warm(a, actor_a); after_warm(b, actor_b)
        hist0, state0, tick_start = actor_a.History(), a.GetState(), a.Tick
        obs_a, rew_a, done_a, act_a, fin_a = [], [], [], [], []
        for t in range(T):
            act = host(actor_a.Step(eps, seed, tick0 + t)).copy()
            assert act.dtype == np.float32
            act_a.append(act)
            r = a.Read()
            obs_a.append(r.Observation.T.copy()); rew_a.append(r.Reward.copy()); done_a.append(a.GetArray("done").copy())
            if bookkeeping:
                fin_a.append((a.GetArray("finished_return").copy(), a.GetArray("finished_length").copy()))
        rec_obs = torch.empty((T, O, n), dtype=torch.float32, device="cuda")
        rec_rew = torch.empty((T, n), dtype=torch.float32, device="cuda")
        rec_done = torch.empty((T, n), dtype=torch.uint8, device="cuda")
        rec_act = torch.empty((T, n), dtype=torch.float32, device="cuda")
        want = []
        if bookkeeping:
            for t in range(T):
                for lane in np.nonzero(done_a[t])[0]:
                    want.append((t, int(lane), float(fin_a[t][0][lane]), int(fin_a[t][1][lane])))
        ep = forms.episode_buffers(T * n) if records_on else None
        b.RolloutFusedDevice(None, T, actions="actor", epsilon=eps, action_seed=seed, action_tick0=tick0, rec_obs=rec_obs, rec_reward=rec_rew,
                             rec_done=rec_done, rec_actions=rec_act, episodes=ep)
        assert np.array_equal(bits(host(rec_act)), bits(np.stack(act_a)))
        assert np.array_equal(bits(host(rec_obs)), bits(np.stack(obs_a)))
        assert np.array_equal(bits(host(rec_rew)), bits(np.stack(rew_a)))
        assert np.array_equal(host(rec_done), np.stack(done_a))
        assert np.array_equal(bits(a.GetState()), bits(b.GetState()))
        assert np.array_equal(a.GetArray("done"), b.GetArray("done"))
        assert a.Tick == b.Tick == tick_start + T
        assert np.array_equal(actor_a.History(), actor_b.History())
        if bookkeeping:
            for k in ("episode_return", "episode_length", "finished_return", "finished_length"):
                assert np.array_equal(a.GetArray(k), b.GetArray(k)), k
        if records_on:
            got, kept, ended = forms.records(ep)
            assert ended == len(want)                                         # count[1]: every episode that ended
            assert kept == ended and got == sorted(want)                      # step, lane, return and length of every record
        if not kw.get("auto_reset"):
            ca, cb = a.Counters(), b.Counters()
            assert ca["stepped_after_done"] == cb["stepped_after_done"] and ca["lane_steps"] == cb["lane_steps"]
        assert np.array_equal(bits(host(actor_a.Step(eps, seed, tick0 + T))), bits(host(actor_b.Step(eps, seed, tick0 + T))))
        return dict(actions=np.stack(act_a), obs=np.stack(obs_a), reward=np.stack(rew_a), done=np.stack(done_a), want=want, hist0=hist0,
                    state0=state0, tick_start=tick_start)
