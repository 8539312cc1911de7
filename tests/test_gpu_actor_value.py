"""GPU checks of the critic a configured actor carries (gym.net_amd/csrc/actor_value.hip: gymnet_vecenv_actor_critic_config,
_actor_critic_load_device, _actor_value_device, _actor_act_value_device and gymnet_vecenv_rollout_fused_value_device).  The value is the
actor's own fmaf chain over the actor's own input, so every comparison with the C twin (tests/_actor_twin.py forward) is twin.same — bit
equality up to the sign of a zero — and every comparison between two device paths is on uint32 views: the stand-alone value against the twin
on the five float32 envs and a float64 CartPole handle, before and after LoadCritic; Act(value=) against Act and Value(); each of the 18
fused forms (tests/_actor_logp_forms.py), with rec_logp and without, against single closed-loop steps, with the rollout that records no
value beside it; one fused rollout per env replayed teacher-forced through the twin and on through AdvantagesDevice against
tests/_advantage_twin.py; EpisodeMemory.Rollout(rec_value=) and actor.Step(repeat=2, value=) against their unfused loops; refusals that
write nothing and the critic's lifetime.  Every test fails without the feature, at the missing method, argument or export.

Batch 321 (257 with the attachments): full waves and a one-lane partial wave.  History 2, actor net [2 * obs_dim, 16, A] as
tests/test_gpu_actor_softmax.py builds it; two critics, [2 * obs_dim, 16, 1] and [2 * obs_dim, 13, 7, 1] — widths that are no multiple of
the kernel's groups of 4 neurons and chunks of 8 inputs, and a depth other than the actor's."""
import ctypes as C

import numpy as np
import pytest

import _actor_forms as aforms
import _actor_logp_forms as forms
import _actor_logp_twin as ltwin
import _actor_twin as twin
import _advantage_twin as atwin
import test_gpu_actor_softmax as soft

pytestmark = pytest.mark.gpu
SEED = soft.SEED
F32 = np.float32
CARTPOLE, MOUNTAINCAR, ACROBOT = soft.CARTPOLE, soft.MOUNTAINCAR, soft.ACROBOT
PENDULUM, MOUNTAINCAR_CONTINUOUS = "Pendulum-v1", "MountainCarContinuous-v0"
OBS = {CARTPOLE: 4, MOUNTAINCAR: 2, ACROBOT: 6, PENDULUM: 3, MOUNTAINCAR_CONTINUOUS: 2}
N, S = soft.N, soft.S
host = soft.host
_net, _at_the_goal = soft._net, soft._at_the_goal
POISON = forms.POISON
ATT = soft.ATT


def _critic(name, deep, seed=11):
    """(widths, flat, pairs) of one of the two critics for this env"""
    O = OBS[name]
    return twin.net(np.random.default_rng([seed, O, int(deep)]), [S * O, 13, 7, 1] if deep else [S * O, 16, 1])


def _u32(t):
    return np.ascontiguousarray(host(t)).view(np.uint32)


def _want_value(critic, actor):
    """the twin's value of the actor's current history, float32 [n]"""
    w, flat, _ = critic
    hist = actor.History()
    return twin.forward(w, flat, hist.reshape(len(hist), -1))[0][:, 0]


def _actor_for(env, name):
    """an actor of this env's kind: the Discrete envs' [2 O, 16, A] net, a Box env's [2 O, 16, 1]"""
    if name in (PENDULUM, MOUNTAINCAR_CONTINUOUS):
        return env.Actor(twin.net(np.random.default_rng(2), [S * OBS[name], 16, 1])[2], history=S)
    return env.Actor(_net(name)[2], history=S)


# ---- 1. the stand-alone value against the twin ------------------------------------------------------------------------------------
@pytest.mark.parametrize("deep", [False, True], ids=["16-1", "13-7-1"])
@pytest.mark.parametrize("name,dtype", [(CARTPOLE, np.float32), (MOUNTAINCAR, np.float32), (ACROBOT, np.float32), (PENDULUM, np.float32),
                                        (MOUNTAINCAR_CONTINUOUS, np.float32), (CARTPOLE, np.float64)],
                         ids=["cartpole", "mountaincar", "acrobot", "pendulum", "mountaincar-continuous", "cartpole-f64"])
def test_value_equals_the_twin(gpu_pkg, name, dtype, deep):
    import torch
    kw = dict(dtype=np.float64) if dtype == np.float64 else {}
    with gpu_pkg.VectorEnv(name, N, seed=SEED, auto_reset=True, **kw) as env:
        env.Reset()
        actor = _actor_for(env, name)
        critic = _critic(name, deep)
        actor.SetCritic(critic[2])
        assert actor.CriticWidths == tuple(int(w) for w in critic[0])
        for t in range(3):                                                   # three warm steps: the ring slot is not 0, the slots differ
            actor.Step(0.5, 77, t)
        hist = actor.History()
        assert (hist[:, 0] != hist[:, 1]).any()
        out = torch.full((N,), POISON, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert actor.Value(out=out) is out
        want = _want_value(critic, actor)
        got = host(out).copy()
        print(f"{name} {np.dtype(dtype).name} critic {critic[0].tolist()}: value range {want.min():.4f} .. {want.max():.4f}, "
              f"{len(np.unique(want))} distinct, bit mismatches {int((got.view(np.uint32) != want.view(np.uint32)).sum())}")
        assert twin.same(got, want), np.nonzero(got != want)[0][:8]
        assert len(np.unique(want)) > N // 2
        assert twin.same(host(actor.Value()), want)                          # ... and into a tensor of its own
        other = _critic(name, deep, seed=12)                                 # other weights of the same widths, through the host ...
        actor.LoadCritic(other[2])
        want2 = _want_value(other, actor)
        assert twin.same(host(actor.Value(out=out)), want2) and not twin.same(want2, want)
        actor.LoadCritic(torch.from_numpy(critic[1]).cuda())                 # ... and the first ones back, device to device
        assert twin.same(host(actor.Value(out=out)), want)
        assert np.array_equal(actor.History(), hist)                         # the critic changes no history
        actor.Step(0.5, 77, 3)                                               # ... and the actor goes on as before


# ---- 2. Act(value=) against the plain calls -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", [("uniform", 1.0), ("softmax", 0.5)], ids=lambda s: s[0])
@pytest.mark.parametrize("name", [CARTPOLE, MOUNTAINCAR, ACROBOT])
def test_act_with_value_equals_the_plain_calls(gpu_pkg, name, setting):
    import torch
    A = forms.DIMS[name][1]
    with gpu_pkg.VectorEnv(name, N, seed=SEED, auto_reset=True) as env:
        env.Reset()
        actor = env.Actor(_net(name)[2], history=S)
        critic = _critic(name, setting[0] == "softmax")
        actor.SetCritic(critic[2])
        actor.SetExploration(*setting)
        for t in range(3):
            actor.Step(0.5, 77, t)
        assert actor.Exploration == setting                                  # SetCritic and Step keep the setting
        logits, logits0 = (torch.full((N, A), -7.0, dtype=torch.float32, device="cuda") for _ in range(2))
        logp, logp0, value = (torch.full((N,), POISON, dtype=torch.float32, device="cuda") for _ in range(3))
        out0 = torch.empty(N, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        want_value = _u32(actor.Value()).copy()
        for eps in (0.0, 0.5, 1.0):
            plain = host(actor.Act(eps, seed=5, tick=3, out=out0, logits=logits0, logp=logp0)).copy()
            got = host(actor.Act(eps, seed=5, tick=3, logits=logits, logp=logp, value=value)).copy()
            assert np.array_equal(got, plain) and np.array_equal(_u32(logits), _u32(logits0)) and np.array_equal(_u32(logp), _u32(logp0))
            assert np.array_equal(_u32(value), want_value)
            value.fill_(POISON)
            torch.cuda.synchronize()
            bare = host(actor.Act(eps, seed=5, tick=3, out=out0)).copy()     # without logp too: the handle's own act kernel runs
            got = host(actor.Act(eps, seed=5, tick=3, value=value)).copy()
            assert np.array_equal(got, bare) and np.array_equal(got, plain)
            assert np.array_equal(_u32(value), want_value)
        assert twin.same(host(value), _want_value(critic, actor))


# ---- 3. all 18 fused forms against single steps -----------------------------------------------------------------------------------
def _fused_value_equals_single_steps(gpu_pkg, row, with_logp, T=12, eps=0.5, seed=99, tick0=1000, warm=3):
    """Handle a runs T x actor.Step(logp=, value=); b one fused rollout with rec_value (and rec_logp, or None); c the same rollout
    without rec_value.  b equals a in everything tests/_actor_logp_forms.py's comparison looks at plus rec_value, bit for bit, its
    poisoned row past T stays poisoned, and c records b's actions and a's logp."""
    import torch
    name = row["env"]
    kw = forms.handle_kwargs(row, limit=5)
    records_on = row["shape"] == "records"
    bookkeeping = bool(kw.get("episode_stats"))
    pairs = _net(name)[2]
    critic = _critic(name, not with_logp)
    setting = ("softmax", 0.5) if with_logp else ("uniform", 1.0)
    n = N
    with gpu_pkg.VectorEnv(name, n, seed=SEED, **kw) as a, gpu_pkg.VectorEnv(name, n, seed=SEED, **kw) as b, gpu_pkg.VectorEnv(name, n, seed=SEED, **kw) as c:
        actors = []
        for env in (a, b, c):
            env.Reset()
            actor = env.Actor(pairs, S)
            actor.SetCritic(critic[2])
            for t in range(warm):
                actor.Step(eps, seed + 1, t)
            _at_the_goal(env)
            actor.Reset()
            actor.SetExploration(*setting)
            actors.append(actor)
        actor_a, actor_b, actor_c = actors
        tick_start = a.Tick
        O = a.ObsDim
        obs_a, rew_a, done_a, act_a, fin_a, logp_a, value_a = [], [], [], [], [], [], []
        lp, vl = (torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(2))
        for t in range(T):
            act_a.append(host(actor_a.Step(eps, seed, tick0 + t, logp=lp, value=vl)).copy())
            logp_a.append(_u32(lp).copy()); value_a.append(_u32(vl).copy())
            r = a.Read()
            obs_a.append(r.Observation.T.copy()); rew_a.append(r.Reward.copy()); done_a.append(a.GetArray("done").copy())
            if bookkeeping:
                fin_a.append((a.GetArray("finished_return").copy(), a.GetArray("finished_length").copy()))
        want = []
        if bookkeeping:
            for t in range(T):
                for lane in np.nonzero(done_a[t])[0]:
                    want.append((t, int(lane), float(fin_a[t][0][lane]), int(fin_a[t][1][lane])))

        def buffers():
            rec = dict(rec_obs=torch.empty((T, O, n), dtype=torch.float32, device="cuda"), rec_reward=torch.empty((T, n), dtype=torch.float32, device="cuda"),
                       rec_done=torch.empty((T, n), dtype=torch.uint8, device="cuda"), rec_actions=torch.empty((T, n), dtype=torch.int32, device="cuda"))
            return rec, torch.full((T + 1, n), POISON, dtype=torch.float32, device="cuda"), torch.full((T + 1, n), POISON, dtype=torch.float32, device="cuda")
        rec_b, lp_b, val_b = buffers()
        rec_c, lp_c, _ = buffers()
        torch.cuda.synchronize()                                             # the fills (torch's stream) end before the handles' streams write
        ep = aforms.episode_buffers(T * n) if records_on else None
        run = dict(actions="actor", epsilon=eps, action_seed=seed, action_tick0=tick0)
        b.RolloutFusedDevice(None, T, episodes=ep, rec_logp=lp_b[:T] if with_logp else None, rec_value=val_b[:T], **run, **rec_b)
        c.RolloutFusedDevice(None, T, rec_logp=lp_c[:T], **run, **rec_c)
        got_v = _u32(val_b)
        assert np.array_equal(got_v[:T], np.stack(value_a)), np.argwhere(got_v[:T] != np.stack(value_a))[:8]
        assert (host(val_b)[T] == F32(POISON)).all()                          # nothing past row T - 1
        if with_logp:
            assert np.array_equal(_u32(lp_b)[:T], np.stack(logp_a)) and (host(lp_b)[T] == F32(POISON)).all()
        else:
            assert (host(lp_b) == F32(POISON)).all()
        assert np.array_equal(_u32(lp_c)[:T], np.stack(logp_a))              # the rollout without rec_value: the same actions and logp
        assert np.array_equal(host(rec_c["rec_actions"]), host(rec_b["rec_actions"]))
        assert np.array_equal(host(rec_b["rec_actions"]), np.stack(act_a))
        assert np.array_equal(_u32(rec_b["rec_obs"]), np.stack(obs_a).astype(F32).view(np.uint32))
        assert np.array_equal(_u32(rec_b["rec_reward"]), np.stack(rew_a).view(np.uint32))
        assert np.array_equal(host(rec_b["rec_done"]), np.stack(done_a))
        for other in (b, c):
            assert np.array_equal(a.GetState().view(np.uint32), other.GetState().view(np.uint32))
            assert np.array_equal(a.GetArray("done"), other.GetArray("done"))
            assert a.Tick == other.Tick == tick_start + T
            if bookkeeping:
                for k in ("episode_return", "episode_length", "finished_return", "finished_length"):
                    assert np.array_equal(a.GetArray(k), other.GetArray(k)), k
        assert np.array_equal(actor_a.History(), actor_b.History()) and np.array_equal(actor_a.History(), actor_c.History())
        if records_on:
            recs, kept, ended = aforms.records(ep)
            assert ended == len(want) and kept == ended and recs == sorted(want)
        if not kw.get("auto_reset"):
            ca, cb = a.Counters(), b.Counters()
            assert ca["stepped_after_done"] == cb["stepped_after_done"] and ca["lane_steps"] == cb["lane_steps"] == (warm + T) * n
            if name == CARTPOLE:
                assert np.array_equal(a.GetArray("steps_beyond_done"), b.GetArray("steps_beyond_done"))
        assert np.array_equal(_u32(actor_a.Value()), _u32(actor_b.Value()))   # the last value, and the next decision
        assert np.array_equal(host(actor_a.Step(eps, seed, tick0 + T)), host(actor_b.Step(eps, seed, tick0 + T)))
        return dict(actions=np.stack(act_a), value=np.stack(value_a), done=np.stack(done_a))


@pytest.mark.parametrize("with_logp", [True, False], ids=["logp", "no-logp"])
@pytest.mark.parametrize("row", forms.FORMS, ids=lambda r: forms.form_id(r).replace("actor_logp_rollout_kernel", "actor_value_rollout_kernel"))
def test_every_form_equals_single_steps(gpu_pkg, row, with_logp):
    """T = 12 with max_episode_steps = 5 on the bookkeeping rows, 3 warm steps so that the ring slot is not 0, MountainCar / Acrobot lanes
    put at the goal: lanes restart inside the rollout.  With rec_logp under ("softmax", 0.5) and the [., 16, 1] critic, without it under
    the default setting and the [., 13, 7, 1] critic."""
    out = _fused_value_equals_single_steps(gpu_pkg, row, with_logp)
    A = forms.DIMS[row["env"]][1]
    assert len(np.unique(out["actions"])) == A
    v = out["value"].view(F32)
    assert np.isfinite(v).all() and len(np.unique(out["value"])) > N
    if row["shape"] != "lean":
        assert (out["done"] & 2).any()
    if row["env"] != CARTPOLE:
        assert (out["done"][0][np.arange(N) % 3 == 0] & 1).all()


# ---- 4. teacher-forced replay, and the loop end to end ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", [CARTPOLE, MOUNTAINCAR, ACROBOT])
def test_a_fused_rollout_replays_teacher_forced_through_the_twin_and_feeds_the_advantages(gpu_pkg, name):
    """From the recorded observations and done bytes the history of every step is rebuilt on the host and the fmaf twin over the critic
    gives rec_value row by row; row T of a [T + 1, n] tensor is the twin's value of the history after the rollout; AdvantagesDevice over
    the device rows equals tests/_advantage_twin.py over their host copy, bit for bit."""
    import torch
    T, eps, aseed, tick0, lane0 = 12, 0.6, 99, 1000, 7
    critic = _critic(name, True)
    with gpu_pkg.VectorEnv(name, N, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=5, lane_offset=lane0) as env:
        obs0 = env.Reset()
        actor = env.Actor(_net(name)[2], history=S)
        actor.SetCritic(critic[2])
        actor.SetExploration("softmax", 0.5)
        rec = dict(rec_obs=torch.empty((T, env.ObsDim, N), dtype=torch.float32, device="cuda"), rec_done=torch.empty((T, N), dtype=torch.uint8, device="cuda"),
                   rec_reward=torch.empty((T, N), dtype=torch.float32, device="cuda"), rec_logp=torch.empty((T, N), dtype=torch.float32, device="cuda"),
                   rec_value=torch.full((T + 1, N), POISON, dtype=torch.float32, device="cuda"))
        torch.cuda.synchronize()
        env.RolloutFusedDevice(None, T, actions="actor", epsilon=eps, action_seed=aseed, action_tick0=tick0, **rec)
        got = {k: host(v).copy() for k, v in rec.items()}
        model = twin.History(obs0, S)
        w, flat, _ = critic
        for t in range(T):
            want = twin.forward(w, flat, model.x())[0][:, 0]
            assert twin.same(got["rec_value"][t], want), (t, np.nonzero(got["rec_value"][t] != want)[0][:8])
            model.push(got["rec_obs"][t].T, got["rec_done"][t])
        assert np.array_equal(actor.History(), model.h)
        assert twin.same(got["rec_value"][T], twin.forward(w, flat, model.x())[0][:, 0])          # the last value
        assert (got["rec_done"] & 2).any() and len(np.unique(got["rec_value"].view(np.uint32))) > N
        adv, ret = (torch.empty((T, N), dtype=torch.float32, device="cuda") for _ in range(2))
        env.AdvantagesDevice(rec["rec_reward"], rec["rec_done"], rec["rec_value"], adv, ret, gamma=0.99, lam=0.95)
        want_adv, want_ret = atwin.gae(got["rec_reward"], got["rec_done"], got["rec_value"][:T], got["rec_value"][T], None, 0.99, 0.95)
        assert atwin.same(host(adv), want_adv) and atwin.same(host(ret), want_ret)
        assert np.isfinite(want_adv).all() and len(np.unique(want_adv)) > N


# ---- 5. attachments ---------------------------------------------------------------------------------------------------------------
def test_actor_step_with_repeat_and_value_equals_the_unfused_loop(gpu_pkg):
    import torch
    n = 257
    pairs = _net(CARTPOLE, seed=4)[2]
    critic = _critic(CARTPOLE, True)
    with gpu_pkg.VectorEnv(CARTPOLE, n, **ATT) as f, gpu_pkg.VectorEnv(CARTPOLE, n, **ATT) as e:
        f.Reset(); e.Reset()
        fa, ea = f.Actor(pairs, history=S), e.Actor(pairs, history=S)
        for actor in (fa, ea):
            actor.SetCritic(critic[2])
            actor.SetExploration("softmax", 0.5)
        vf, ve, lf, le = (torch.full((n,), POISON, dtype=torch.float32, device="cuda") for _ in range(4))
        torch.cuda.synchronize()
        seen = set()
        for d in range(12):
            got = host(fa.Step(0.5, 77, d, repeat=2, logp=lf, value=vf)).copy()
            want_value = _want_value(critic, ea)
            ea.Value(out=ve)
            want = ea.Act(0.5, 77, d, logp=le)
            e.StepRepeatDevice(want, 2)
            ea.Push()
            assert np.array_equal(got, host(want)), d
            assert np.array_equal(_u32(vf), _u32(ve)) and np.array_equal(_u32(lf), _u32(le)), d
            assert twin.same(host(vf), want_value), d
            seen.update(np.unique(_u32(vf)).tolist())
            assert np.array_equal(f.GetState(), e.GetState()) and f.Tick == e.Tick == 1 + 3 * (d + 1)
            assert np.array_equal(fa.History(), ea.History()), d
        assert len(seen) > n and (f.GetArray("finished_length") > 0).any()


def test_memory_rollout_with_rec_value_equals_single_steps_and_pushes(gpu_pkg):
    import torch
    n, T = 257, 24
    pairs = _net(CARTPOLE, seed=5)[2]
    critic = _critic(CARTPOLE, False)
    snaps = []
    for fused in (False, True):
        with gpu_pkg.VectorEnv(CARTPOLE, n, **ATT) as env:
            env.Reset()
            actor = env.Actor(pairs, history=S)
            actor.SetCritic(critic[2])
            actor.SetExploration("softmax", 0.5)
            mem = env.EpisodeMemory(capacity=5, max_length=9, history=S, rollout_chunk=16)
            rec = torch.full((T + 1, n), POISON, dtype=torch.float32, device="cuda")
            logp = torch.full((T, n), POISON, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            if fused:
                taken = host(mem.Rollout(T, actions="actor", action_seed=77, action_tick0=1000, epsilon=0.5, rec_logp=logp, rec_value=rec)).copy()
            else:
                rows = []
                for t in range(T):
                    acts = actor.Step(0.5, 77, 1000 + t, logp=logp[t], value=rec[t])
                    mem.Push(acts)
                    rows.append(host(acts).copy())
                actor.Value(out=rec[T])
                taken = np.stack(rows)
            x, a, onehot, r = (host(v) for v in mem.BuildDataset("params", min_episodes=0, reward=True))
            snaps.append(dict(taken=taken, value=_u32(rec).copy(), logp=_u32(logp).copy(), stats=mem.Stats(), x=x, a=a, onehot=onehot, r=r, state=env.GetState(),
                              hist=actor.History(), tick=env.Tick, last=_want_value(critic, actor)))
    a, b = snaps
    assert a["stats"] == b["stats"] and a["stats"]["ended"] > 5 and a["tick"] == b["tick"]
    assert np.array_equal(a["taken"], b["taken"]) and len(np.unique(a["taken"])) == 2
    v = b["value"].view(F32)
    assert np.isfinite(v).all() and len(np.unique(b["value"])) > n and twin.same(v[T], b["last"])
    for k in ("value", "logp", "x", "a", "onehot", "r", "state", "hist"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


# ---- 6. refusals write nothing; the critic's lifetime ------------------------------------------------------------------------------
def _spec(capi, T, source, eps=0.5, seed=99, tick0=1000, **rec):
    return capi.RolloutSpec(struct_size=C.sizeof(capi.RolloutSpec), action_source=source, steps=T, action_stride=0, ring=1, action_seed=seed,
                            action_tick0=tick0, epsilon=eps, **{k: C.c_void_p(v.data_ptr()) for k, v in rec.items()})


def test_refusals_write_nothing(gpu_pkg):
    import importlib
    import torch
    capi = importlib.import_module(gpu_pkg.__name__ + "._capi")
    T = 4

    def buffers(n):
        b = dict(acts=torch.full((n,), -7, dtype=torch.int32, device="cuda"), logp=torch.full((n,), POISON, dtype=torch.float32, device="cuda"),
                 value=torch.full((n,), POISON, dtype=torch.float32, device="cuda"), rec=torch.full((T, n), POISON, dtype=torch.float32, device="cuda"),
                 rec_logp=torch.full((T, n), POISON, dtype=torch.float32, device="cuda"), rec_act=torch.full((T, n), -7, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        return b

    def intact(b):
        return all(bool((b[k] == (-7 if k in ("acts", "rec_act") else POISON)).all()) for k in b)

    def p(t, off=0):
        return C.c_void_p(t.data_ptr() + off)

    def value(lib, h, b, off=0):
        return lib.gymnet_vecenv_actor_value_device(h, p(b["value"], off))

    def act_value(lib, h, b, eps=0.5, off=0):
        return lib.gymnet_vecenv_actor_act_value_device(h, p(b["acts"]), None, p(b["logp"]), p(b["value"], off), C.c_float(eps), 5, 3)

    def fused_value(lib, h, b, source, d_actions=None, off=0, logp_off=0):
        spec = _spec(capi, T, source, d_rec_actions=b["rec_act"])
        if d_actions is not None:
            spec.d_actions = C.c_void_p(d_actions.data_ptr())
        return lib.gymnet_vecenv_rollout_fused_value_device(h, C.byref(spec), p(b["rec_logp"], logp_off), p(b["rec"], off))

    def unchanged(env, actor, state, tick, hist):
        env.Sync()
        return np.array_equal(env.GetState().view(np.uint32), state.view(np.uint32)) and env.Tick == tick and np.array_equal(actor.History(), hist)

    with gpu_pkg.VectorEnv(PENDULUM, N, seed=SEED) as env:                                  # a Box actor: Value serves it, the rest does not
        env.Reset()
        lib, h = env._lib, env._h
        b = buffers(N)
        critic = _critic(PENDULUM, False)
        flat, widths = critic[1], critic[0]
        assert lib.gymnet_vecenv_actor_critic_config(h, 2, widths.ctypes.data_as(C.c_void_p), flat.ctypes.data_as(C.c_void_p), flat.size) == capi.ERR_INVALID_ARG   # no actor
        assert value(lib, h, b) == capi.ERR_INVALID_ARG and fused_value(lib, h, b, capi.ACTIONS_ACTOR) == capi.ERR_INVALID_ARG
        actor = _actor_for(env, PENDULUM)
        state, tick, hist = env.GetState(), env.Tick, actor.History()
        assert value(lib, h, b) == capi.ERR_INVALID_ARG and b"critic" in lib.gymnet_last_error()            # no critic yet
        actor.SetCritic(critic[2])
        assert act_value(lib, h, b) == capi.ERR_INVALID_ARG and b"Box" in lib.gymnet_last_error()
        assert fused_value(lib, h, b, capi.ACTIONS_ACTOR) == capi.ERR_INVALID_ARG and b"Box" in lib.gymnet_last_error()
        assert intact(b) and unchanged(env, actor, state, tick, hist)
        with pytest.raises(ValueError, match="Box"):
            actor.Act(0.5, 5, 3, value=b["value"])
        with pytest.raises(ValueError, match="Box"):
            env.RolloutFusedDevice(None, T, actions="actor", rec_value=b["rec"])
        actor.SetPolicy("tanh", "gaussian", 0.1)                                            # keeps the critic
        assert value(lib, h, b) == capi.OK and twin.same(host(b["value"]), _want_value(critic, actor))
        actor.Step(0.5, 5, 3)                                                               # the Box actor still works
    with gpu_pkg.VectorEnv(CARTPOLE, N, seed=SEED, auto_reset=True) as env:
        env.Reset()
        lib, h = env._lib, env._h
        b = buffers(N)
        critic = _critic(CARTPOLE, True)
        widths, flat = critic[0], critic[1]
        wp, fp = widths.ctypes.data_as(C.c_void_p), flat.ctypes.data_as(C.c_void_p)
        actor = env.Actor(_net(CARTPOLE)[2], history=S)
        ring = torch.zeros((T, N), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        state, tick, hist = env.GetState(), env.Tick, actor.History()
        # no critic
        assert value(lib, h, b) == capi.ERR_INVALID_ARG and b"critic" in lib.gymnet_last_error()
        assert act_value(lib, h, b) == capi.ERR_INVALID_ARG and b"critic" in lib.gymnet_last_error()
        assert fused_value(lib, h, b, capi.ACTIONS_ACTOR) == capi.ERR_INVALID_ARG and b"critic" in lib.gymnet_last_error()
        assert lib.gymnet_vecenv_actor_critic_load_device(h, p(b["rec"]), flat.size) == capi.ERR_INVALID_ARG
        with pytest.raises(ValueError, match="critic"):
            env.RolloutFusedDevice(None, T, actions="actor", rec_value=b["rec"])
        # a refused config changes nothing: a first width, a last width, a limit, a count, a depth
        bad = [np.array(wd, np.int32) for wd in ([9, 13, 7, 1], [8, 13, 7, 2], [8, 65, 1], [8, 13, 0, 1])]
        for wd in bad:
            assert lib.gymnet_vecenv_actor_critic_config(h, len(wd) - 1, wd.ctypes.data_as(C.c_void_p), fp, flat.size) == capi.ERR_INVALID_ARG, wd
        assert lib.gymnet_vecenv_actor_critic_config(h, 3, wp, fp, flat.size - 1) == capi.ERR_INVALID_ARG
        assert lib.gymnet_vecenv_actor_critic_config(h, 5, wp, fp, flat.size) == capi.ERR_INVALID_ARG
        assert lib.gymnet_vecenv_actor_critic_config(h, 3, None, fp, flat.size) == capi.ERR_INVALID_ARG
        assert value(lib, h, b) == capi.ERR_INVALID_ARG
        actor.SetCritic(critic[2])
        for wd in bad:                                                                      # ... also over a configured critic, which stays
            assert lib.gymnet_vecenv_actor_critic_config(h, len(wd) - 1, wd.ctypes.data_as(C.c_void_p), fp, flat.size) == capi.ERR_INVALID_ARG, wd
        assert lib.gymnet_vecenv_actor_critic_load_device(h, p(b["rec"]), flat.size + 1) == capi.ERR_INVALID_ARG
        assert lib.gymnet_vecenv_actor_critic_load_device(h, None, flat.size) == capi.ERR_INVALID_ARG
        assert intact(b)
        assert twin.same(host(actor.Value()), _want_value(critic, actor))
        # an action source other than the actor, misaligned and null pointers, the act call's own refusals
        for source in (capi.ACTIONS_RING, capi.ACTIONS_SAMPLE, capi.ACTIONS_EPSILON_GREEDY, 7):
            assert fused_value(lib, h, b, source, ring) == capi.ERR_INVALID_ARG, source
        assert fused_value(lib, h, b, capi.ACTIONS_ACTOR, off=2) == capi.ERR_INVALID_ARG
        assert fused_value(lib, h, b, capi.ACTIONS_ACTOR, logp_off=2) == capi.ERR_INVALID_ARG
        assert value(lib, h, b, off=2) == capi.ERR_INVALID_ARG and lib.gymnet_vecenv_actor_value_device(h, None) == capi.ERR_INVALID_ARG
        assert act_value(lib, h, b, off=2) == capi.ERR_INVALID_ARG
        assert act_value(lib, h, b, eps=1.5) == capi.ERR_INVALID_ARG
        assert lib.gymnet_vecenv_actor_act_value_device(h, None, None, None, p(b["value"]), C.c_float(0.5), 5, 3) == capi.ERR_INVALID_ARG
        assert lib.gymnet_vecenv_actor_act_value_device(h, p(b["acts"]), None, p(b["logp"], 2), p(b["value"]), C.c_float(0.5), 5, 3) == capi.ERR_INVALID_ARG
        assert lib.gymnet_vecenv_rollout_fused_value_device(h, None, None, p(b["rec"])) == capi.ERR_INVALID_ARG            # a null spec
        spec = _spec(capi, T, capi.ACTIONS_ACTOR, eps=1.5)                                  # the rollout's own checks apply
        assert lib.gymnet_vecenv_rollout_fused_value_device(h, C.byref(spec), None, p(b["rec"])) == capi.ERR_INVALID_ARG
        spec = _spec(capi, 0, capi.ACTIONS_ACTOR)                                           # steps == 0 writes nothing and is no error
        assert lib.gymnet_vecenv_rollout_fused_value_device(h, C.byref(spec), p(b["rec_logp"]), p(b["rec"])) == capi.OK
        assert intact(b) and unchanged(env, actor, state, tick, hist)
        # a stale history: one step without a push
        env.StepDevice(actor.Act(0.5, 5, 3))
        state, tick = env.GetState(), env.Tick
        assert value(lib, h, b) == capi.ERR_INVALID_ARG and b"stale" in lib.gymnet_last_error()
        assert act_value(lib, h, b) == capi.ERR_INVALID_ARG and b"stale" in lib.gymnet_last_error()
        assert fused_value(lib, h, b, capi.ACTIONS_ACTOR) == capi.ERR_INVALID_ARG and b"stale" in lib.gymnet_last_error()
        assert intact(b) and unchanged(env, actor, state, tick, hist)
        actor.Push()                                                                        # ... and after the push all three serve again
        assert value(lib, h, b) == capi.OK and act_value(lib, h, b) == capi.OK and fused_value(lib, h, b, capi.ACTIONS_ACTOR) == capi.OK
        env.Sync()
        assert not any(bool((b[k] == POISON).any()) for k in ("value", "logp", "rec", "rec_logp"))
        # the value pointer belongs to the one call that was given it: the plain and the logp rollout after it leave it alone
        b = buffers(N)
        env.RolloutFusedDevice(None, T, actions="actor", epsilon=0.5, rec_actions=b["rec_act"])
        env.RolloutFusedDevice(None, T, actions="actor", epsilon=0.5, rec_logp=b["rec_logp"])
        env.Sync()
        assert bool((b["rec"] == POISON).all()) and not bool((b["rec_logp"] == POISON).any())
        # the lifetime: Load, Reset, SetExploration keep the critic; removing it refuses a value; a new actor drops it
        actor.Load(_net(CARTPOLE, seed=3)[2]); actor.Reset(); actor.SetExploration("softmax", 2.0)
        assert twin.same(host(actor.Value()), _want_value(critic, actor))
        actor.SetCritic(None)
        b = buffers(N)
        assert actor.CriticWidths is None and value(lib, h, b) == capi.ERR_INVALID_ARG and b"critic" in lib.gymnet_last_error()
        assert fused_value(lib, h, b, capi.ACTIONS_ACTOR) == capi.ERR_INVALID_ARG
        with pytest.raises(ValueError, match="critic"):
            actor.Value()
        actor.SetCritic(critic[2])
        assert value(lib, h, b) == capi.OK
        fresh = env.Actor(_net(CARTPOLE)[2], history=S)                                     # a new env.Actor(...) drops the critic
        b = buffers(N)
        assert fresh.CriticWidths is None and value(lib, h, b) == capi.ERR_INVALID_ARG and b"critic" in lib.gymnet_last_error()
        assert act_value(lib, h, b) == capi.ERR_INVALID_ARG and fused_value(lib, h, b, capi.ACTIONS_ACTOR) == capi.ERR_INVALID_ARG
        env.Sync()
        assert intact(b)
        fresh.Step(0.5, 5, 3)                                                               # ... and acts on without one
    with gpu_pkg.VectorEnv(CARTPOLE, N, seed=SEED, auto_reset=True, dtype=np.float64) as env:          # float64: value serves, the fused rollout does not
        env.Reset()
        lib, h = env._lib, env._h
        b = buffers(N)
        actor = env.Actor(_net(CARTPOLE)[2], history=S)
        actor.SetCritic(_critic(CARTPOLE, False)[2])
        assert fused_value(lib, h, b, capi.ACTIONS_ACTOR) == capi.ERR_UNSUPPORTED
        env.Sync()
        assert intact(b)
        assert act_value(lib, h, b) == capi.OK
