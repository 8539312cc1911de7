"""The recipe table of the fused actor rollout's kernels under an exploration setting other than the default (helper module, not a
conftest), and the comparison every recipe runs.

actor_softmax.hip compiles actor_softmax_rollout_kernel<Env, AUTORESET, EXTRAS, RECORDS> in 18 forms — CartPole, MountainCar and Acrobot x
auto-reset on / off x {lean, bookkeeping, bookkeeping with episode records}, the shapes of tests/_actor_forms.py — and takes explore and
1 / temperature as kernel arguments, so a setting adds no form.  Each row names one form the way the assembly demangles it and says how to
reach it through the public API: the env, the handle's auto_reset, its shape, and Actor.SetExploration("softmax", ...) on the handle's
actor: under "uniform" actor.hip's kernel of the same shape runs instead.  tests/test_actor_softmax_host.py pins the table to the
compiled set; tests/test_gpu_actor_softmax.py runs every row under each of SETTINGS.

fused_equals_single_steps is tests/_actor_forms.py's comparison with one more hook: after_warm(env, actor) runs on both handles once their
actors exist and the warm steps are done — where the setting is set."""
import numpy as np

import _actor_forms as forms

ENVS, SHAPES = forms.ENVS, forms.SHAPES
DIMS = {"CartPole-v1": (4, 2), "MountainCar-v0": (2, 3), "Acrobot-v1": (6, 3)}           # env -> (obs_dim, actions)
# (explore, temperature): the default, which must stay what it was, and two softmax settings
SETTINGS = [("uniform", 1.0), ("softmax", 1.0), ("softmax", 0.5)]


def _b(v):
    return "true" if v else "false"


FORMS = [dict(kernel=f"actor_softmax_rollout_kernel<{env},{_b(ar)},{_b(SHAPES[shape][0])},{_b(SHAPES[shape][1])}>", env=gym, auto_reset=ar,
              shape=shape)
         for env, gym in ENVS.items() for ar in (True, False) for shape in SHAPES]
ACT_KERNELS = ("actor_softmax_act_kernel<2>", "actor_softmax_act_kernel<4>", "actor_softmax_act_kernel<6>")
# the actor.hip sibling of a kernel of this unit
SIBLING = {row["kernel"]: row["kernel"].replace("actor_softmax_rollout_kernel", "actor_rollout_kernel") for row in FORMS}
SIBLING.update({k: k.replace("actor_softmax_act_kernel", "actor_act_kernel") for k in ACT_KERNELS})


def form_id(row):
    return row["kernel"]


def handle_kwargs(row, limit):
    kw = dict(auto_reset=row["auto_reset"])
    if row["shape"] != "lean":
        kw.update(episode_stats=True, max_episode_steps=limit)
    return kw


def fused_equals_single_steps(gpu_pkg, name, n, T, kw, records_on, pairs, S=4, eps=0.5, seed=99, tick0=1000, warm=0, after_warm=None,
                              env_seed=0xAC7, lane_offset=0):
    """Handle a runs T x actor.Step (Act, StepDevice, Push), its twin b one fused actor rollout; the recorded actions, observations, rewards
    and dones, the state, done bytes, tick, history, episode statistics, the episode records (as sets, return and length included),
    count[1] and, without auto-reset, the counters are equal, and both accept the next single step.  Returns what handle a saw, and the
    fused rollout's recordings (rec_obs, rec_actions) with the history and state it started from."""
    import torch
    host = forms.host
    bookkeeping = bool(kw.get("episode_stats"))
    assert not records_on or bookkeeping
    with gpu_pkg.VectorEnv(name, n, seed=env_seed, lane_offset=lane_offset, **kw) as a, \
            gpu_pkg.VectorEnv(name, n, seed=env_seed, lane_offset=lane_offset, **kw) as b:
        a.Reset(); b.Reset()
        O = a.ObsDim
        actor_a, actor_b = a.Actor(pairs, S), b.Actor(pairs, S)
        for t in range(warm):
            actor_a.Step(eps, seed + 1, t); actor_b.Step(eps, seed + 1, t)
        if after_warm:
            after_warm(a, actor_a); after_warm(b, actor_b)
        hist0, state0, tick_start = actor_a.History(), a.GetState(), a.Tick
        obs_a, rew_a, done_a, act_a, fin_a = [], [], [], [], []
        for t in range(T):
            act_a.append(host(actor_a.Step(eps, seed, tick0 + t)).copy())
            r = a.Read()
            obs_a.append(r.Observation.T.copy()); rew_a.append(r.Reward.copy()); done_a.append(a.GetArray("done").copy())
            if bookkeeping:
                fin_a.append((a.GetArray("finished_return").copy(), a.GetArray("finished_length").copy()))
        rec_obs = torch.empty((T, O, n), dtype=torch.float32, device="cuda")
        rec_rew = torch.empty((T, n), dtype=torch.float32, device="cuda")
        rec_done = torch.empty((T, n), dtype=torch.uint8, device="cuda")
        rec_act = torch.empty((T, n), dtype=torch.int32, device="cuda")
        want = []
        if bookkeeping:
            for t in range(T):
                for lane in np.nonzero(done_a[t])[0]:
                    want.append((t, int(lane), float(fin_a[t][0][lane]), int(fin_a[t][1][lane])))
        ep = forms.episode_buffers(T * n) if records_on else None
        b.RolloutFusedDevice(None, T, actions="actor", epsilon=eps, action_seed=seed, action_tick0=tick0, rec_obs=rec_obs, rec_reward=rec_rew,
                             rec_done=rec_done, rec_actions=rec_act, episodes=ep)
        kernel = b.KernelName()
        assert np.array_equal(host(rec_act), np.stack(act_a))
        assert np.array_equal(host(rec_obs).view(np.uint32), np.stack(obs_a).astype(np.float32).view(np.uint32))
        assert np.array_equal(host(rec_rew).view(np.uint32), np.stack(rew_a).view(np.uint32))
        assert np.array_equal(host(rec_done), np.stack(done_a))
        assert np.array_equal(a.GetState().view(np.uint32), b.GetState().view(np.uint32))
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
            assert ca["stepped_after_done"] == cb["stepped_after_done"] and ca["lane_steps"] == cb["lane_steps"] == (warm + T) * n
            if name == "CartPole-v1":
                assert np.array_equal(a.GetArray("steps_beyond_done"), b.GetArray("steps_beyond_done"))
        assert np.array_equal(host(actor_a.Step(eps, seed, tick0 + T)), host(actor_b.Step(eps, seed, tick0 + T)))
        return dict(actions=np.stack(act_a), obs=np.stack(obs_a), reward=np.stack(rew_a), done=np.stack(done_a), want=want, hist0=hist0,
                    state0=state0, tick_start=tick_start, kernel=kernel)
