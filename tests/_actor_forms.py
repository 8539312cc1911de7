"""The recipe table of the fused actor rollout's kernels (helper module, not a conftest), and the comparison every recipe runs.

actor.hip compiles actor_rollout_kernel<Env, AUTORESET, EXTRAS, RECORDS> in 18 forms: three envs x auto-reset on / off x {lean,
bookkeeping, bookkeeping with episode records} (launch_actor_rollout_env).  Each row of FORMS names one form the way the assembly
demangles it and says how to reach it through the public API: the env, the handle's auto_reset, and its shape — "lean" (no bookkeeping
flag), "book" (episode_stats=True, max_episode_steps=LIMIT) or "records" ("book" plus an episodes= dict in the rollout call).
tests/test_actor_host.py pins the table to the compiled set; tests/test_gpu_actor_forms.py runs every row.

fused_equals_single_steps is the comparison itself: one handle runs T x (Act, StepDevice, Push), its twin one fused rollout with
actions="actor", and everything either leaves behind is compared bit for bit."""
import numpy as np

import _actor_twin as twin

ENVS = {"CartPole": "CartPole-v1", "MountainCar": "MountainCar-v0", "Acrobot": "Acrobot-v1"}
SHAPES = {"lean": (False, False), "book": (True, False), "records": (True, True)}        # shape -> (EXTRAS, RECORDS)
LIMIT = 25           # max_episode_steps of the bookkeeping rows: below the 40 steps of the forms test, so MountainCar and Acrobot lanes end too
HIDDEN = {"CartPole-v1": [50, 20], "MountainCar-v0": [13, 7], "Acrobot-v1": [50, 20]}   # the runner's hidden widths


def _b(v):
    return "true" if v else "false"


FORMS = [dict(kernel=f"actor_rollout_kernel<{env},{_b(ar)},{_b(SHAPES[shape][0])},{_b(SHAPES[shape][1])}>", env=gym, auto_reset=ar, shape=shape)
         for env, gym in ENVS.items() for ar in (True, False) for shape in SHAPES]


def form_id(row):
    return row["kernel"]


def handle_kwargs(row, limit=LIMIT):
    kw = dict(auto_reset=row["auto_reset"])
    if row["shape"] != "lean":
        kw.update(episode_stats=True, max_episode_steps=limit)
    return kw


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def episode_buffers(cap):
    import torch
    return dict(step=torch.empty(max(cap, 1), dtype=torch.int32, device="cuda"), lane=torch.empty(max(cap, 1), dtype=torch.int32, device="cuda"),
                ret=torch.empty(max(cap, 1), dtype=torch.float32, device="cuda"), length=torch.empty(max(cap, 1), dtype=torch.int32, device="cuda"),
                capacity=cap, count=torch.zeros(2, dtype=torch.int32, device="cuda"))


def records(ep):
    """(sorted (step, lane, return, length) tuples of the records kept, count[0], count[1])"""
    cnt = host(ep["count"]).astype(np.int64)
    m = int(cnt[0])
    got = sorted(zip(host(ep["step"])[:m].tolist(), host(ep["lane"])[:m].tolist(), host(ep["ret"])[:m].tolist(), host(ep["length"])[:m].tolist()))
    return got, int(cnt[0]), int(cnt[1])


def fused_equals_single_steps(gpu_pkg, name, n, T, kw, records_on, pairs, S=4, eps=0.3, seed=99, tick0=1000, full=False, prepare=None,
                              capacity=None, env_seed=0xAC7, warm=0, per_handle=None, configure=None):
    """Handle a runs T x actor.Step (Act, StepDevice, Push), its twin b one fused actor rollout; asserts that the recorded actions,
    observations, rewards and dones, the state, done bytes, tick, history, episode statistics, the episode records (as sets, return and
    length included), count[1], CartPole's steps_beyond_done and the stepped-after-done counter of a handle without auto-reset, and (full)
    the last step's done list and terminal observations are equal, and that both accept the next single step.  prepare(env) runs on each
    handle after Reset and before its actor is configured; warm: closed-loop single steps both handles take first, so the rollout starts
    from a ring slot other than 0 and from histories whose slots differ.  capacity None: T * n records (at most one per lane and step);
    "exact": as many as the single steps ended; a number below that: the records kept are that many distinct true ones.  Returns what
    handle a saw: dict(actions, obs, reward, done [T, ...], finished [(return, length)] per step, want = the records the steps imply,
    got / kept / ended = the fused rollout's records and its two counts).
    per_handle(k), k = 0 for a and 1 for b: what the two handles cannot share, as dict(kwargs=more VectorEnv arguments of that handle
    alone (caller-owned observation buffers), after=a callable(env) run on it once everything has been compared (the buffers' sentinels)).
    configure(env, actor) runs on each handle once its actor exists (an exploration setting).  Both default to nothing."""
    import torch
    bookkeeping = bool(kw.get("episode_stats"))
    assert not records_on or bookkeeping
    own = [per_handle(k) for k in (0, 1)] if per_handle else [{}, {}]
    with gpu_pkg.VectorEnv(name, n, seed=env_seed, **kw, **own[0].get("kwargs", {})) as a, \
            gpu_pkg.VectorEnv(name, n, seed=env_seed, **kw, **own[1].get("kwargs", {})) as b:
        a.Reset(); b.Reset()
        if prepare:
            prepare(a); prepare(b)
        O = a.ObsDim
        actor_a, actor_b = a.Actor(pairs, S), b.Actor(pairs, S)
        if configure:
            configure(a, actor_a); configure(b, actor_b)
        for t in range(warm):
            actor_a.Step(eps, seed + 1, t); actor_b.Step(eps, seed + 1, t)
        obs_a, rew_a, done_a, act_a, fin_a = [], [], [], [], []
        for t in range(T):
            act_a.append(host(actor_a.Step(eps, seed, tick0 + t)).copy())
            r = a.Read()
            obs_a.append(r.Observation.T.copy()); rew_a.append(r.Reward.copy()); done_a.append(a.GetArray("done").copy())
            if bookkeeping:                                              # the finished episodes' (return, length) of this step
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
        ep = episode_buffers({None: T * n, "exact": len(want)}.get(capacity, capacity)) if records_on else None
        b.RolloutFusedDevice(None, T, actions="actor", epsilon=eps, action_seed=seed, action_tick0=tick0, rec_obs=rec_obs, rec_reward=rec_rew,
                             rec_done=rec_done, rec_actions=rec_act, episodes=ep)
        assert np.array_equal(host(rec_act), np.stack(act_a))
        assert np.array_equal(host(rec_obs).view(np.uint32), np.stack(obs_a).astype(np.float32).view(np.uint32))
        assert np.array_equal(host(rec_rew).view(np.uint32), np.stack(rew_a).view(np.uint32))
        assert np.array_equal(host(rec_done), np.stack(done_a))
        assert np.array_equal(a.GetState().view(np.uint32), b.GetState().view(np.uint32))
        assert np.array_equal(a.GetArray("done"), b.GetArray("done"))
        assert a.Tick == b.Tick
        assert np.array_equal(actor_a.History(), actor_b.History())
        if bookkeeping:
            for k in ("episode_return", "episode_length", "finished_return", "finished_length"):
                assert np.array_equal(a.GetArray(k), b.GetArray(k)), k
        got, kept, ended = [], 0, 0
        if records_on:
            got, kept, ended = records(ep)
            assert ended == len(want)                                         # count[1]: every episode that ended
            if ep["capacity"] >= len(want):
                assert kept == ended and got == sorted(want)                  # step, lane, return and length of every record
            else:
                assert kept == ep["capacity"] and set(got) <= set(want) and len(set(got)) == kept
        if not kw.get("auto_reset"):
            ca, cb = a.Counters(), b.Counters()
            assert ca["stepped_after_done"] == cb["stepped_after_done"] and ca["lane_steps"] == cb["lane_steps"] == (warm + T) * n
            if name == "CartPole-v1":
                assert np.array_equal(a.GetArray("steps_beyond_done"), b.GetArray("steps_beyond_done"))
        if full:                                                                  # the last step's done list and terminal observations
            assert np.array_equal(a.GetArray("final_obs").view(np.uint32), b.GetArray("final_obs").view(np.uint32))
            assert np.array_equal(np.sort(a.DoneLanes()), np.sort(b.DoneLanes()))
            ra, rb = a.DoneRecords(), b.DoneRecords()
            ka, kb = np.argsort(ra["lanes"]), np.argsort(rb["lanes"])
            for k in ("lanes", "return", "length", "final_obs"):
                assert np.array_equal(ra[k][ka], rb[k][kb]), k
        # the history is current after the fused rollout: the next single step is accepted on both
        assert np.array_equal(host(actor_a.Step(eps, seed, tick0 + T)), host(actor_b.Step(eps, seed, tick0 + T)))
        out = dict(actions=np.stack(act_a), obs=np.stack(obs_a), reward=np.stack(rew_a), done=np.stack(done_a), finished=fin_a, want=want,
                   got=got, kept=kept, ended=ended)
        if not kw.get("auto_reset"):
            out["stepped_after_done"] = ca["stepped_after_done"]
            if name == "CartPole-v1":
                out["steps_beyond_done"] = a.GetArray("steps_beyond_done")      # (after the extra step above)
        for env, o in zip((a, b), own):
            if o.get("after"):
                o["after"](env)
        return out
