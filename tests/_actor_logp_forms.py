"""The recipe table of the fused actor rollout's kernels that also record the log-probability of every action taken (helper module, not a
conftest), and the comparison every recipe runs.

actor_logp.hip compiles actor_logp_rollout_kernel<Env, AUTORESET, EXTRAS, RECORDS> in 18 forms — CartPole, MountainCar and Acrobot x
auto-reset on / off x {lean, bookkeeping, bookkeeping with episode records}, the shapes of tests/_actor_forms.py — and takes explore and
1 / temperature as kernel arguments, so a setting adds no form: a request for logp runs this unit under the default setting too.  Each row
names one form the way the assembly demangles it and says how to reach it through the public API: the env, the handle's auto_reset, its
shape, and RolloutFusedDevice(actions="actor", rec_logp=...).  tests/test_actor_logp_host.py pins the table to the compiled set;
tests/test_gpu_actor_logp.py runs every row under each of SETTINGS.

fused_equals_single_steps: handle a runs T x actor.Step(logp=...), its twin b one fused rollout with rec_logp; the recorded
log-probabilities are equal as bits — and so is everything tests/_actor_softmax_forms.py's comparison looks at, which this one repeats
with the logp calls in place of the plain ones."""
import numpy as np

import _actor_forms as forms
import _actor_softmax_forms as sforms

ENVS, SHAPES, DIMS, SETTINGS = sforms.ENVS, sforms.SHAPES, sforms.DIMS, sforms.SETTINGS
handle_kwargs = sforms.handle_kwargs
POISON = -7.25                                     # what the rec_logp buffer holds before the launch (no logp is above +0)


def _b(v):
    return "true" if v else "false"


FORMS = [dict(kernel=f"actor_logp_rollout_kernel<{env},{_b(ar)},{_b(SHAPES[shape][0])},{_b(SHAPES[shape][1])}>", env=gym, auto_reset=ar, shape=shape)
         for env, gym in ENVS.items() for ar in (True, False) for shape in SHAPES]
ACT_KERNELS = ("actor_logp_act_kernel<2>", "actor_logp_act_kernel<4>", "actor_logp_act_kernel<6>")
# the actor_softmax.hip sibling of a kernel of this unit
SIBLING = {row["kernel"]: row["kernel"].replace("actor_logp_rollout_kernel", "actor_softmax_rollout_kernel") for row in FORMS}
SIBLING.update({k: k.replace("actor_logp_act_kernel", "actor_softmax_act_kernel") for k in ACT_KERNELS})


def form_id(row):
    return row["kernel"]


def fused_equals_single_steps(gpu_pkg, name, n, T, kw, records_on, pairs, S=4, eps=0.5, seed=99, tick0=1000, warm=0, after_warm=None,
                              env_seed=0xAC7, lane_offset=0):
    """tests/_actor_softmax_forms.py's fused_equals_single_steps with logp: handle a runs T x actor.Step(logp=) (Act with logp, StepDevice,
    Push), its twin b one fused actor rollout with rec_logp [T + 1, N], whose last row is poison and stays poison.  Returns what handle a
    saw, with the log-probabilities (uint32 bits) and the fused rollout's start."""
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
        obs_a, rew_a, done_a, act_a, fin_a, logp_a = [], [], [], [], [], []
        lp = torch.empty(n, dtype=torch.float32, device="cuda")
        for t in range(T):
            act_a.append(host(actor_a.Step(eps, seed, tick0 + t, logp=lp)).copy())
            logp_a.append(host(lp).view(np.uint32).copy())
            r = a.Read()
            obs_a.append(r.Observation.T.copy()); rew_a.append(r.Reward.copy()); done_a.append(a.GetArray("done").copy())
            if bookkeeping:
                fin_a.append((a.GetArray("finished_return").copy(), a.GetArray("finished_length").copy()))
        rec_obs = torch.empty((T, O, n), dtype=torch.float32, device="cuda")
        rec_rew = torch.empty((T, n), dtype=torch.float32, device="cuda")
        rec_done = torch.empty((T, n), dtype=torch.uint8, device="cuda")
        rec_act = torch.empty((T, n), dtype=torch.int32, device="cuda")
        rec_all = torch.full((T + 1, n), POISON, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()                                             # the fill (torch's stream) ends before the handle's stream writes
        want = []
        if bookkeeping:
            for t in range(T):
                for lane in np.nonzero(done_a[t])[0]:
                    want.append((t, int(lane), float(fin_a[t][0][lane]), int(fin_a[t][1][lane])))
        ep = forms.episode_buffers(T * n) if records_on else None
        b.RolloutFusedDevice(None, T, actions="actor", epsilon=eps, action_seed=seed, action_tick0=tick0, rec_obs=rec_obs, rec_reward=rec_rew,
                             rec_done=rec_done, rec_actions=rec_act, episodes=ep, rec_logp=rec_all[:T])
        kernel = b.KernelName()
        got = host(rec_all)
        assert np.array_equal(got[:T].view(np.uint32), np.stack(logp_a)), np.argwhere(got[:T].view(np.uint32) != np.stack(logp_a))[:8]
        assert (got[T] == np.float32(POISON)).all()                          # nothing past row T - 1
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
            recs, kept, ended = forms.records(ep)
            assert ended == len(want)                                         # count[1]: every episode that ended
            assert kept == ended and recs == sorted(want)                     # step, lane, return and length of every record
        if not kw.get("auto_reset"):
            ca, cb = a.Counters(), b.Counters()
            assert ca["stepped_after_done"] == cb["stepped_after_done"] and ca["lane_steps"] == cb["lane_steps"] == (warm + T) * n
            if name == "CartPole-v1":
                assert np.array_equal(a.GetArray("steps_beyond_done"), b.GetArray("steps_beyond_done"))
        assert np.array_equal(host(actor_a.Step(eps, seed, tick0 + T)), host(actor_b.Step(eps, seed, tick0 + T)))
        return dict(actions=np.stack(act_a), logp=np.stack(logp_a), obs=np.stack(obs_a), reward=np.stack(rew_a), done=np.stack(done_a), want=want,
                    hist0=hist0, state0=state0, tick_start=tick_start, kernel=kernel)
