"""GPU checks of V(terminal observation) on time-limit rows (gym.net_amd/csrc/actor_boot.hip: gymnet_vecenv_actor_boot_device,
gymnet_vecenv_rollout_fused_value_boot_device, gymnet_vecenv_rollout_fused_box_boot_device).  The boot is the critic's own fmaf chain over
ring rows 1 .. S-1 and the terminal observation, so every comparison with the C twin (tests/_actor_twin.py forward, through
tests/_actor_boot_cases.py want_boot) is twin.same — bit equality up to the sign of a zero — and every comparison between two device paths
is on uint32 views: the stand-alone Boot() against the twin on the five float32 envs and a float64 CartPole handle, with and without
auto_reset; each of the 20 fused forms, with and without rec_logp / rec_logd, against single closed-loop steps, with a handle without
final_obs and the rollout that records no boot beside it; one rollout per env on through AdvantagesDevice against tests/_advantage_twin.py;
EpisodeMemory.Rollout(rec_boot=) and actor.Step(repeat=2, boot=) against their unfused loops; refusals that write nothing.  Every test
fails without the feature, at the missing method, argument or export.

Batch 321 (257 with the attachments), T = 12, history 2, max_episode_steps = 7 with the running episode lengths staggered per lane by
tests/_actor_boot_cases.py, whose coverage counts (rows with d = 1, 2, 3; waves with every, no and some lanes truncated) are asserted
wherever the table is used."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _actor_boot_cases as cases
import _actor_forms as aforms
import _actor_twin as twin
import _advantage_twin as atwin
import test_gpu_actor_value as val

pytestmark = pytest.mark.gpu
SEED = val.SEED
F32 = np.float32
N, S, T = cases.N, cases.S, cases.T
POISON = cases.POISON
host, _u32, _actor_for = val.host, val._u32, val._actor_for
CARTPOLE, MOUNTAINCAR, ACROBOT, PENDULUM, MCC = "CartPole-v1", "MountainCar-v0", "Acrobot-v1", "Pendulum-v1", "MountainCarContinuous-v0"
BOX_POLICY = ("tanh", "gaussian", 0.3)


def _prepared(env, name, critic, warm=3, eps=0.5, seed=100):
    """an actor with the critic on a reset handle: three warm closed-loop steps (the ring slot is not 0), then the case table"""
    env.Reset()
    actor = _actor_for(env, name)
    actor.SetCritic(critic[2])
    for t in range(warm):
        actor.Step(eps, seed, t)
    cases.place(env, name)
    actor.Reset()
    if actor.IsBox:
        actor.SetPolicy(*BOX_POLICY)
    return actor


def _terminal_obs(env):
    """[n, O]: the post-step observation before any reset, as the stand-alone call reads it"""
    return env.GetArray("final_obs").T if env.AutoReset else env.Read().Observation


# ---- 1. the stand-alone boot against the twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto-reset", "no-reset"])
@pytest.mark.parametrize("deep", [False, True], ids=["16-1", "13-7-1"])
@pytest.mark.parametrize("name,dtype", [(CARTPOLE, np.float32), (MOUNTAINCAR, np.float32), (ACROBOT, np.float32), (PENDULUM, np.float32),
                                        (MCC, np.float32), (CARTPOLE, np.float64)],
                         ids=["cartpole", "mountaincar", "acrobot", "pendulum", "mountaincar-continuous", "cartpole-f64"])
def test_boot_equals_the_twin(gpu_pkg, name, dtype, deep, auto_reset):
    import torch
    kw = cases.handle_kwargs(auto_reset, final_obs=auto_reset, **(dict(dtype=np.float64) if dtype == np.float64 else {}))
    critic = cases.critic(name, deep)
    with gpu_pkg.VectorEnv(name, N, seed=SEED, **kw) as env:
        actor = _prepared(env, name, critic)
        out = torch.full((N,), POISON, dtype=torch.float32, device="cuda")
        model = twin.History(np.zeros((N, env.ObsDim), F32), S)
        model.h = actor.History()
        dones, distinct, slots_differ = [], 0, False
        for t in range(T):
            hist = actor.History()
            env.StepDevice(actor.Act(0.5, 77, 100 + t))
            done, term, tick = env.GetArray("done"), _terminal_obs(env), env.Tick
            out.fill_(POISON)
            torch.cuda.synchronize()                                         # the fill (torch's stream) ends before the handle's stream writes
            assert actor.Boot(out=out) is out
            got = host(out).copy()
            want = cases.want_boot(critic, hist, term, done)
            trunc = (done & 2) != 0
            assert twin.same(got, want), (t, np.nonzero(got != want)[0][:8])
            assert (got.view(np.uint32)[~trunc] == 0).all()                  # +0.0f on every row without bit 1: the poison is gone
            if t == 0:
                assert twin.same(host(actor.Boot()), want)                   # ... and into a tensor of its own
            assert np.array_equal(actor.History(), hist) and env.Tick == tick
            slots_differ |= bool((hist[trunc, 0] != hist[trunc, 1]).any())
            distinct += len(np.unique(want[trunc]))
            actor.Push()                                                     # ... and the push goes on as it would have
            model.push(env.Read().Observation, done)
            assert np.array_equal(actor.History(), model.h), t
            dones.append(done)
        cov = cases.coverage(np.stack(dones))
        print(f"{name} {np.dtype(dtype).name} auto_reset={auto_reset} critic {critic[0].tolist()}: {cov}, {distinct} distinct boot values")
        cases.assert_covered(cov, name)
        assert slots_differ and distinct > cov["d2"] // 2


# ---- 2. all 20 fused forms against single steps -----------------------------------------------------------------------------------
def _spec(capi, steps, eps, seed, tick0, **rec):
    return capi.RolloutSpec(struct_size=C.sizeof(capi.RolloutSpec), action_source=capi.ACTIONS_ACTOR, steps=steps, action_stride=0, ring=1, action_seed=seed,
                            action_tick0=tick0, epsilon=eps, **{k: C.c_void_p(v.data_ptr()) for k, v in rec.items()})


def _fused_boot_equals_single_steps(gpu_pkg, row, with_lp, eps=0.5, seed=99, tick0=1000):
    """Handle a (final_obs=True) runs T x actor.Step(logp / logd=, value=, boot=); b one fused rollout with rec_boot; c, without final_obs,
    the same rollout; d the rollout with rec_value and no rec_boot.  b equals a in everything the sibling comparisons look at plus rec_boot,
    bit for bit; the poisoned rows past T stay poisoned; c leaves b's bits; d leaves b's bits in everything but the boot it never wrote."""
    import torch
    capi = importlib.import_module(gpu_pkg.__name__ + "._capi")
    name, box, ar, records_on = row["env"], row["box"], row["auto_reset"], row["records"]
    critic = cases.critic(name, not with_lp)
    n = N
    # (the library keeps final observations on auto-reset handles only: without auto_reset the terminal observation stays current)
    envs = [gpu_pkg.VectorEnv(name, n, seed=SEED, **cases.handle_kwargs(ar, final_obs=fo and ar)) for fo in (True, True, False, True)]
    try:
        actors = [_prepared(env, name, critic, eps=eps, seed=seed + 1) for env in envs]
        if not box:
            for actor in actors:
                actor.SetExploration(*(("softmax", 0.5) if with_lp else ("uniform", 1.0)))
        a, b, c, d = envs
        actor_a, actor_b = actors[:2]
        tick_start, O = a.Tick, a.ObsDim
        obs_a, rew_a, done_a, act_a, fin_a, lp_a, value_a, boot_a, want_b = [], [], [], [], [], [], [], [], []
        lp, vl, bt = (torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(3))
        for t in range(T):
            hist = actor_a.History()
            if box:
                actor_a.Value(out=vl)
                act_a.append(host(actor_a.Step(eps, seed, tick0 + t, logd=lp, boot=bt)).copy())
            else:
                act_a.append(host(actor_a.Step(eps, seed, tick0 + t, logp=lp, value=vl, boot=bt)).copy())
            lp_a.append(_u32(lp).copy()); value_a.append(_u32(vl).copy()); boot_a.append(_u32(bt).copy())
            r = a.Read()
            obs_a.append(r.Observation.T.copy()); rew_a.append(r.Reward.copy()); done_a.append(a.GetArray("done").copy())
            fin_a.append((a.GetArray("finished_return").copy(), a.GetArray("finished_length").copy()))
            want_b.append(cases.want_boot(critic, hist, _terminal_obs(a), done_a[-1]))
        done_a = np.stack(done_a)
        want = [(t, int(lane), float(fin_a[t][0][lane]), int(fin_a[t][1][lane])) for t in range(T) for lane in np.nonzero(done_a[t])[0]]

        def buffers():
            rec = dict(rec_obs=torch.empty((T, O, n), dtype=torch.float32, device="cuda"), rec_reward=torch.empty((T, n), dtype=torch.float32, device="cuda"),
                       rec_done=torch.empty((T, n), dtype=torch.uint8, device="cuda"),
                       rec_actions=torch.empty((T, n), dtype=torch.float32 if box else torch.int32, device="cuda"))
            return (rec,) + tuple(torch.full((T + 1, n), POISON, dtype=torch.float32, device="cuda") for _ in range(3))
        bufs = [buffers() for _ in range(3)]
        torch.cuda.synchronize()                                             # the fills (torch's stream) end before the handles' streams write
        eps_ = [aforms.episode_buffers(T * n) if records_on else None for _ in range(3)]

        def fused(env, ep, rec, lp_t, val_t, boot_t):
            """the rollout through the Python method; a Box actor without rec_logd through the C call (Python asks for rec_logd there)"""
            if box and not with_lp:
                assert not records_on or ep is not None
                spec = _spec(capi, T, eps, seed, tick0, **{"d_" + k: v for k, v in rec.items()})
                if ep is not None:
                    spec.d_ep_step, spec.d_ep_lane, spec.d_ep_return, spec.d_ep_length, spec.d_ep_count = (
                        C.c_void_p(ep[k].data_ptr()) for k in ("step", "lane", "ret", "length", "count"))
                    spec.ep_capacity = ep["capacity"]
                p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
                assert env._lib.gymnet_vecenv_rollout_fused_box_boot_device(env._h, C.byref(spec), None, p(val_t), p(boot_t)) == capi.OK
                return
            kw = dict(rec_logd=lp_t[:T]) if box else dict(rec_logp=lp_t[:T] if with_lp else None)
            env.RolloutFusedDevice(None, T, actions="actor", epsilon=eps, action_seed=seed, action_tick0=tick0, episodes=ep, rec_value=val_t[:T],
                                   rec_boot=None if boot_t is None else boot_t[:T], **kw, **rec)
        for env, ep, (rec, lp_t, val_t, boot_t), with_boot in zip((b, c, d), eps_, bufs, (True, True, False)):
            fused(env, ep, rec, lp_t, val_t, boot_t if with_boot else None)
        (rec_b, lp_b, val_b, boot_b), (rec_c, lp_c, val_c, boot_c), (rec_d, lp_d, val_d, boot_d) = bufs
        got = _u32(boot_b)
        assert np.array_equal(got[:T], np.stack(boot_a)), np.argwhere(got[:T] != np.stack(boot_a))[:8]
        assert twin.same(host(boot_b)[:T], np.stack(want_b))                 # ... which is the definition
        assert (got[:T][(done_a & 2) == 0] == 0).all()                       # +0.0f where no time limit struck
        assert (host(boot_b)[T] == F32(POISON)).all() and (host(val_b)[T] == F32(POISON)).all()        # nothing past row T - 1
        assert np.array_equal(_u32(val_b)[:T], np.stack(value_a))
        if with_lp:
            assert np.array_equal(_u32(lp_b)[:T], np.stack(lp_a)) and (host(lp_b)[T] == F32(POISON)).all()
        else:
            assert (host(lp_b) == F32(POISON)).all()
        assert np.array_equal(_u32(rec_b["rec_actions"]), np.stack(act_a).view(np.uint32))
        assert np.array_equal(_u32(rec_b["rec_obs"]), np.stack(obs_a).astype(F32).view(np.uint32))
        assert np.array_equal(_u32(rec_b["rec_reward"]), np.stack(rew_a).view(np.uint32))
        assert np.array_equal(host(rec_b["rec_done"]), done_a)
        for other_rec, other_lp, other_val in ((rec_c, lp_c, val_c), (rec_d, lp_d, val_d)):      # c: no FINAL_OBS; d: the forwarding target
            for k in rec_b:
                assert np.array_equal(host(other_rec[k]).view(np.uint8), host(rec_b[k]).view(np.uint8)), k
            assert np.array_equal(_u32(other_lp), _u32(lp_b)) and np.array_equal(_u32(other_val), _u32(val_b))
        assert np.array_equal(_u32(boot_c), got)
        assert (host(boot_d) == F32(POISON)).all()                           # no rec_boot: never written
        for other in (b, c, d):
            assert np.array_equal(a.GetState().view(np.uint32), other.GetState().view(np.uint32))
            assert np.array_equal(a.GetArray("done"), other.GetArray("done"))
            assert a.Tick == other.Tick == tick_start + T
            for k in ("episode_return", "episode_length", "finished_return", "finished_length"):
                assert np.array_equal(a.GetArray(k), other.GetArray(k)), k
            if not ar:
                ca, co = a.Counters(), other.Counters()
                assert ca["stepped_after_done"] == co["stepped_after_done"] and ca["lane_steps"] == co["lane_steps"]
                if name == CARTPOLE:
                    assert np.array_equal(a.GetArray("steps_beyond_done"), other.GetArray("steps_beyond_done"))
        if ar:
            assert np.array_equal(a.GetArray("final_obs").view(np.uint32), b.GetArray("final_obs").view(np.uint32))
        for other in actors[1:]:
            assert np.array_equal(actor_a.History(), other.History())
        if records_on:
            for ep in eps_:
                recs, kept, ended = aforms.records(ep)
                assert ended == len(want) and kept == ended and recs == sorted(want)
        assert np.array_equal(_u32(actor_a.Value()), _u32(actor_b.Value()))  # the last value, and the next decision
        assert np.array_equal(host(actor_a.Step(eps, seed, tick0 + T)), host(actor_b.Step(eps, seed, tick0 + T)))
        return done_a
    finally:
        for env in envs:
            env.Close()


@pytest.mark.parametrize("with_lp", [True, False], ids=["with-logp", "value-only"])
@pytest.mark.parametrize("row", cases.FORMS, ids=cases.form_id)
def test_every_form_equals_single_steps(gpu_pkg, row, with_lp):
    done = _fused_boot_equals_single_steps(gpu_pkg, row, with_lp)
    cov = cases.coverage(done)
    print(f"{row['kernel']}: {cov}")
    cases.assert_covered(cov, row["env"])
    if row["auto_reset"]:
        assert ((done & 2) != 0).sum(axis=0).max() >= 2                      # a lane truncates, restarts and truncates again


# ---- 3. through GAE ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [CARTPOLE, MOUNTAINCAR, ACROBOT, PENDULUM, MCC])
def test_a_rollout_with_boot_feeds_the_advantages(gpu_pkg, name):
    """RolloutFusedDevice(rec_value [T + 1], rec_boot) -> AdvantagesDevice(boot=) against the advantage twin fed the boot the actor twin
    gives for the recorded rows; without boot= the advantages differ on a truncated row."""
    import torch
    critic = cases.critic(name, True)
    box = name in cases.BOX.values()
    with gpu_pkg.VectorEnv(name, N, seed=SEED, **cases.handle_kwargs(True, final_obs=True)) as env, \
            gpu_pkg.VectorEnv(name, N, seed=SEED, **cases.handle_kwargs(True, final_obs=True)) as ref:
        actor, actor_r = _prepared(env, name, critic), _prepared(ref, name, critic)
        O = env.ObsDim
        rew = torch.empty((T, N), dtype=torch.float32, device="cuda")
        done = torch.empty((T, N), dtype=torch.uint8, device="cuda")
        values = torch.empty((T + 1, N), dtype=torch.float32, device="cuda")
        lp, boot = (torch.full((T, N), POISON, dtype=torch.float32, device="cuda") for _ in range(2))
        adv, ret, adv0, ret0 = (torch.empty((T, N), dtype=torch.float32, device="cuda") for _ in range(4))
        torch.cuda.synchronize()
        kw = dict(rec_logd=lp) if box else dict(rec_logp=lp)
        env.RolloutFusedDevice(None, T, actions="actor", epsilon=0.5, action_seed=5, action_tick0=50, rec_reward=rew, rec_done=done, rec_value=values,
                               rec_boot=boot, **kw)
        env.AdvantagesDevice(rew, done, values, adv, ret, gamma=0.99, lam=0.95, boot=boot)
        env.AdvantagesDevice(rew, done, values, adv0, ret0, gamma=0.99, lam=0.95)
        # the twin's boot, from the same closed loop taken one step at a time on a second handle
        want_boot = []
        for t in range(T):
            hist = actor_r.History()
            actor_r.Step(0.5, 5, 50 + t)            # (Push has run: the done bytes and the dense final observations are still this step's)
            want_boot.append(cases.want_boot(critic, hist, ref.GetArray("final_obs").T, ref.GetArray("done")))
        want_boot = np.stack(want_boot)
        d = host(done)
        assert twin.same(host(boot), want_boot)
        cases.assert_covered(cases.coverage(d), name)
        want_adv, want_ret = atwin.gae(host(rew), d, host(values)[:T], host(values)[T], np.where(want_boot == 0, F32(0), want_boot), 0.99, 0.95)
        assert atwin.same(host(adv), want_adv) and atwin.same(host(ret), want_ret)
        only_trunc = d == 2
        assert only_trunc.any() and (host(adv)[only_trunc] != host(adv0)[only_trunc]).any()      # the array is consumed


# ---- 4. the other routes ----------------------------------------------------------------------------------------------------------------
ATT = dict(seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=cases.LIMIT, final_obs=True)


def test_actor_step_with_repeat_and_boot_equals_the_unfused_loop(gpu_pkg):
    import torch
    n = cases.N_ATT
    critic = cases.critic(CARTPOLE, False)
    with gpu_pkg.VectorEnv(CARTPOLE, n, **ATT) as f, gpu_pkg.VectorEnv(CARTPOLE, n, **ATT) as e:
        fa, ea = _prepared(f, CARTPOLE, critic), _prepared(e, CARTPOLE, critic)
        bf, be = (torch.full((n,), POISON, dtype=torch.float32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        truncated = 0
        for dcs in range(T):
            hist = ea.History()
            got = host(fa.Step(0.5, 77, dcs, repeat=2, boot=bf)).copy()
            want = ea.Act(0.5, 77, dcs)
            e.StepRepeatDevice(want, 2)
            done = e.GetArray("done")
            ea.Boot(out=be)
            assert twin.same(host(be), cases.want_boot(critic, hist, e.GetArray("final_obs").T, done)), dcs
            ea.Push()
            assert np.array_equal(got, host(want)) and np.array_equal(_u32(bf), _u32(be)), dcs
            assert np.array_equal(f.GetState(), e.GetState()) and f.Tick == e.Tick
            assert np.array_equal(fa.History(), ea.History()), dcs
            truncated += int(((done & 2) != 0).sum())
        assert truncated > 0


def test_memory_rollout_with_boot_equals_single_steps_and_pushes(gpu_pkg):
    import torch
    n, steps = cases.N_ATT, 24
    critic = cases.critic(CARTPOLE, True)
    snaps = []
    for fused in (False, True):
        with gpu_pkg.VectorEnv(CARTPOLE, n, **ATT) as env:
            actor = _prepared(env, CARTPOLE, critic)
            mem = env.EpisodeMemory(capacity=5, max_length=cases.LIMIT, history=S, rollout_chunk=16)
            value, boot = (torch.full((steps, n), POISON, dtype=torch.float32, device="cuda") for _ in range(2))
            torch.cuda.synchronize()
            if fused:
                taken = host(mem.Rollout(steps, actions="actor", action_seed=77, action_tick0=1000, epsilon=0.5, rec_value=value, rec_boot=boot)).copy()
            else:
                taken = []
                for t in range(steps):
                    acts = actor.Step(0.5, 77, 1000 + t, value=value[t], boot=boot[t])
                    mem.Push(acts)
                    taken.append(host(acts).copy())
                taken = np.stack(taken)
            snaps.append(dict(taken=taken, value=_u32(value).copy(), boot=_u32(boot).copy(), stats=mem.Stats(), state=env.GetState(), hist=actor.History(),
                              tick=env.Tick))
    a, b = snaps
    assert a["stats"] == b["stats"] and a["stats"]["ended"] > 5
    for k in ("taken", "value", "boot", "state", "hist"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    assert a["tick"] == b["tick"] and (a["boot"] != 0).any() and (a["boot"] == 0).any()


# ---- 5. refusals that write nothing -----------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(gpu_pkg):
    import torch
    capi = importlib.import_module(gpu_pkg.__name__ + "._capi")
    n = cases.N_ATT
    critic = cases.critic(CARTPOLE, False)
    buf = torch.full((T + 1, n), POISON, dtype=torch.float32, device="cuda")
    val_t = torch.full((T + 1, n), POISON, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def untouched():
        return bool((host(buf) == F32(POISON)).all() and (host(val_t) == F32(POISON)).all())

    def spec_for(env):
        return _spec(capi, T, 0.5, 5, 50)
    with gpu_pkg.VectorEnv(CARTPOLE, n, **ATT) as env:
        lib, h = env._lib, env._h
        env.Reset()
        assert lib.gymnet_vecenv_actor_boot_device(h, p(buf)) == capi.ERR_INVALID_ARG                      # no actor
        actor = _actor_for(env, CARTPOLE)
        acts = actor.Act(0.5, 1, 0)
        env.StepDevice(acts)
        assert lib.gymnet_vecenv_actor_boot_device(h, p(buf)) == capi.ERR_INVALID_ARG                      # no critic
        with pytest.raises(ValueError, match="critic"):
            actor.Boot()
        spec = spec_for(env)
        actor.Push()
        assert lib.gymnet_vecenv_rollout_fused_value_boot_device(h, C.byref(spec), None, p(val_t), p(buf)) == capi.ERR_INVALID_ARG     # no critic
        actor.SetCritic(critic[2])
        assert lib.gymnet_vecenv_rollout_fused_value_boot_device(h, C.byref(spec), None, None, p(buf)) == capi.ERR_INVALID_ARG         # no rec_value
        with pytest.raises(ValueError, match="rec_value"):
            env.RolloutFusedDevice(None, T, actions="actor", rec_boot=buf[:T])
        assert lib.gymnet_vecenv_rollout_fused_value_boot_device(h, C.byref(spec), None, p(val_t), p(buf, 2)) == capi.ERR_INVALID_ARG  # misaligned
        assert lib.gymnet_vecenv_rollout_fused_box_boot_device(h, C.byref(spec), p(val_t), p(val_t), p(buf)) == capi.ERR_INVALID_ARG   # a Box call, a Discrete actor
        assert lib.gymnet_vecenv_actor_boot_device(h, p(buf)) == capi.ERR_INVALID_ARG                      # no step since the push
        env.StepDevice(actor.Act(0.5, 1, 1))
        assert lib.gymnet_vecenv_actor_boot_device(h, None) == capi.ERR_INVALID_ARG                        # null
        assert lib.gymnet_vecenv_actor_boot_device(h, p(buf, 2)) == capi.ERR_INVALID_ARG                   # misaligned
        assert untouched()
        hist, tick = actor.History(), env.Tick
        first = host(actor.Boot()).copy()                                    # ... and the call they all refused; it leaves the state a push needs,
        assert np.array_equal(host(actor.Boot()).view(np.uint32), first.view(np.uint32))                   # so a second one writes the same row
        assert np.array_equal(actor.History(), hist) and env.Tick == tick
        actor.Push()
        for _ in range(2):                                                   # Boot() twice in a row with no step between: both refused
            assert lib.gymnet_vecenv_actor_boot_device(h, p(buf)) == capi.ERR_INVALID_ARG
        assert untouched()
    # no time limit: nothing can be truncated
    with gpu_pkg.VectorEnv(CARTPOLE, n, seed=SEED, auto_reset=True, episode_stats=True, final_obs=True) as env:
        env.Reset()
        actor = _actor_for(env, CARTPOLE)
        actor.SetCritic(critic[2])
        spec = spec_for(env)
        assert env._lib.gymnet_vecenv_rollout_fused_value_boot_device(env._h, C.byref(spec), None, p(val_t), p(buf)) == capi.ERR_INVALID_ARG
        env.StepDevice(actor.Act(0.5, 1, 0))
        assert env._lib.gymnet_vecenv_actor_boot_device(env._h, p(buf)) == capi.ERR_INVALID_ARG
        actor.Push()
    # auto_reset without final_obs: Boot() has nowhere to read the terminal observation; the fused call does not need it (test 2)
    with gpu_pkg.VectorEnv(CARTPOLE, n, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=cases.LIMIT) as env:
        env.Reset()
        actor = _actor_for(env, CARTPOLE)
        actor.SetCritic(critic[2])
        env.StepDevice(actor.Act(0.5, 1, 0))
        assert env._lib.gymnet_vecenv_actor_boot_device(env._h, p(buf)) == capi.ERR_INVALID_ARG
        with pytest.raises(Exception, match="FINAL_OBS"):
            actor.Boot(out=buf[0])
        actor.Push()
    # a Discrete pointer on a Box handle
    with gpu_pkg.VectorEnv(PENDULUM, n, **ATT) as env:
        env.Reset()
        actor = _actor_for(env, PENDULUM)
        actor.SetCritic(cases.critic(PENDULUM, False)[2])
        actor.SetPolicy(*BOX_POLICY)
        spec = spec_for(env)
        assert env._lib.gymnet_vecenv_rollout_fused_value_boot_device(env._h, C.byref(spec), None, p(val_t), p(buf)) == capi.ERR_INVALID_ARG
        assert env._lib.gymnet_vecenv_rollout_fused_box_boot_device(env._h, C.byref(spec), None, None, p(buf)) == capi.ERR_INVALID_ARG
        with pytest.raises(ValueError):
            env.RolloutFusedDevice(None, T, actions="actor", rec_value=val_t[:T], rec_boot=buf[:T])       # (a Box actor without rec_logd: not built)
    assert untouched()
