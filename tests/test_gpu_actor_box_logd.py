"""GPU checks of the log-density a Box actor records and of the critic's value inside its fused rollout
(gym.net_amd/csrc/actor_box_logd.hip: gymnet_vecenv_actor_box_act_logd_device, gymnet_vecenv_rollout_fused_box_logd_device) on Pendulum
and MountainCarContinuous.  The log-density's arithmetic is specified operation for operation, so Act(logd=) equals the NumPy twin
(tests/_actor_box_logd_twin.py) bit for bit, from the action the call returns and the greedy action the call without exploration
returns; actions and raw outputs are the same bits with and without the request.  Each of the 12 fused forms
(tests/_actor_box_logd_forms.py) under two policies records what T x (Value, Act(logd=), StepDevice, Push) write, bit for bit, with
rec_logd alone and with rec_value alone (through the C call) beside it; one Pendulum rollout's values go against the fmaf twin and on
through AdvantagesDevice; refusals write nothing and leave the handle usable.  Every test fails without the feature, at the missing
argument or export.

Batch 321: full waves and a one-lane partial wave.  History 2, actor net [2 * obs_dim, 16, 1] scaled as tests/test_gpu_actor_box_policy.py
scales it, critics [2 * obs_dim, 16, 1] and [2 * obs_dim, 13, 7, 1], T = 12."""
import ctypes as C

import numpy as np
import pytest

import _actor_box_forms as box
import _actor_box_logd_forms as forms
import _actor_box_logd_twin as dtwin
import _actor_box_policy_twin as ptwin
import _actor_forms as aforms
import _actor_twin as twin
import _advantage_twin as atwin
import test_gpu_actor_box_policy as pol

pytestmark = pytest.mark.gpu
SEED = pol.SEED
F32 = np.float32
PENDULUM, MCC = pol.PENDULUM, pol.MCC
OBS_DIM = pol.OBS_DIM
N, S, T = 321, 2, 12
POISON = forms.POISON
host, bits, _net, _near_goal = pol.host, pol.bits, pol._net, pol._near_goal
ACT_SEED, ACT_TICK = 77, 12
# the coin at epsilon = 0 is word B <= 255: no lane of this (seed, tick) has such a word, so Act(0.0) returns the greedy action on every lane
# (nor of the refusal test's act call and the four steps of its rollout)
for _seed, _tick in ((ACT_SEED, ACT_TICK), (5, 3), (99, 1000), (99, 1001), (99, 1002), (99, 1003)):
    assert not ptwin.explore_mask(ptwin.words(_seed, 0, _tick, N)[1], 0.0).any(), (_seed, _tick)


def _critic(name, deep, seed=11):
    """(widths, flat, pairs) of one of the two critics for this env"""
    O = OBS_DIM[name]
    return twin.net(np.random.default_rng([seed, O, int(deep)]), [S * O, 13, 7, 1] if deep else [S * O, 16, 1])


def _want_value(critic, actor):
    w, flat, _ = critic
    hist = actor.History()
    return twin.forward(w, flat, hist.reshape(len(hist), -1))[0][:, 0]


def _c_bits(sigma):
    return dtwin.constants(sigma)[1].view(np.uint32)


# ---- 1. Act(logd=) against the twin, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", forms.ACT_POLICIES, ids=lambda p: "-".join(map(str, p)))
@pytest.mark.parametrize("name", [PENDULUM, MCC])
def test_act_logd_equals_the_twin(gpu_pkg, name, policy):
    import torch
    head, explore, sigma = policy
    low, high = box.BOUNDS[name]
    with gpu_pkg.VectorEnv(name, N, seed=SEED, auto_reset=True) as env:
        x0 = twin.History(env.Reset(), S).x()
        actor = env.Actor(_net(name, x0)[2], history=S)
        actor.SetPolicy(head, explore, sigma)
        wb = ptwin.words(ACT_SEED, 0, ACT_TICK, N)[1]
        assert not ptwin.explore_mask(wb, 0.0).any()
        g = host(actor.Act(0.0, seed=ACT_SEED, tick=ACT_TICK)).copy()        # the greedy action after the head, on every lane
        raw, raw0 = (torch.full((N, 1), -7.0, dtype=torch.float32, device="cuda") for _ in range(2))
        logd = torch.full((N,), POISON, dtype=torch.float32, device="cuda")
        out0 = torch.empty(N, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()                                             # the fills (torch's stream) end before the handle's stream writes
        for eps in (0.0, 0.5, 1.0):
            plain = host(actor.Act(eps, seed=ACT_SEED, tick=ACT_TICK, out=out0, logits=raw0)).copy()
            a = host(actor.Act(eps, seed=ACT_SEED, tick=ACT_TICK, logits=raw, logd=logd)).copy()
            assert a.dtype == np.float32 and np.array_equal(bits(a), bits(plain))          # the same bits with and without the request
            assert np.array_equal(bits(host(raw)), bits(host(raw0)))
            got = host(logd).copy()
            want = dtwin.logd(a, g, sigma)
            mask = ptwin.explore_mask(wb, eps)
            print(f"{name} {policy} eps {eps}: explore {int(mask.sum())}/{N}  bit mismatches {int((bits(got) != bits(want)).sum())}  "
                  f"logd {np.nanmin(got):.4f} .. {np.nanmax(got):.4f}  distinct {len(np.unique(bits(got)))}")
            assert np.array_equal(bits(got), bits(want)), np.nonzero(bits(got) != bits(want))[0][:8]
            assert not (bits(a) != bits(g))[~mask].any()
            assert (bits(got)[~mask] == _c_bits(sigma)).all()                 # greedy lanes get exactly c
            assert np.isfinite(got).all() and np.all((a >= low) & (a <= high))
            if eps == 0.0:
                assert not mask.any()
            if eps == 0.5:
                assert mask.any() and (~mask).any()
            if eps == 1.0:
                assert mask.all()
                if explore == "gaussian":
                    assert len(np.unique(bits(got))) > N // 2
            logd.fill_(POISON)
            torch.cuda.synchronize()


# ---- 2. all 12 fused forms against single steps -----------------------------------------------------------------------------------------
def _spec(capi, steps, source, eps, seed, tick0, **rec):
    return capi.RolloutSpec(struct_size=C.sizeof(capi.RolloutSpec), action_source=source, steps=steps, action_stride=0, ring=1, action_seed=seed,
                            action_tick0=tick0, epsilon=eps, **{k: C.c_void_p(v.data_ptr()) for k, v in rec.items()})


def _fused_logd_equals_single_steps(gpu_pkg, row, policy, eps=0.5, seed=99, tick0=1000, warm=3):
    """Handle a runs T x (Value, actor.Step(logd=)); b one fused rollout with rec_logd and rec_value; c the same rollout with rec_logd
    alone; d with rec_value alone, through the C call.  b equals a in everything tests/_actor_box_forms.py's comparison looks at plus
    both record streams, bit for bit; the poisoned rows past T stay poisoned; c and d record b's streams and leave the other one alone."""
    import importlib
    import torch
    capi = importlib.import_module(gpu_pkg.__name__ + "._capi")
    name = row["env"]
    kw = forms.handle_kwargs(row, limit=5)
    records_on = row["shape"] == "records"
    bookkeeping = bool(kw.get("episode_stats"))
    pairs = _net(name)[2]
    critic = _critic(name, policy[1] == "sample")
    n = N
    envs = [gpu_pkg.VectorEnv(name, n, seed=SEED, **kw) for _ in range(4)]
    try:
        actors = []
        for env in envs:
            env.Reset()
            actor = env.Actor(pairs, S)
            actor.SetCritic(critic[2])
            for t in range(warm):
                actor.Step(eps, seed + 1, t)
            _near_goal(env)
            actor.Reset()
            actor.SetPolicy(*policy)
            actors.append(actor)
        a, b, c, d = envs
        actor_a, actor_b, actor_c, actor_d = actors
        name0 = b.KernelName()
        tick_start, O = a.Tick, a.ObsDim
        obs_a, rew_a, done_a, act_a, fin_a, logd_a, value_a = [], [], [], [], [], [], []
        ld, vl = (torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(2))
        for t in range(T):
            actor_a.Value(out=vl)
            value_a.append(bits(host(vl)).copy())
            act_a.append(host(actor_a.Step(eps, seed, tick0 + t, logd=ld)).copy())
            logd_a.append(bits(host(ld)).copy())
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
                       rec_done=torch.empty((T, n), dtype=torch.uint8, device="cuda"), rec_actions=torch.empty((T, n), dtype=torch.float32, device="cuda"))
            return rec, torch.full((T + 1, n), POISON, dtype=torch.float32, device="cuda"), torch.full((T + 1, n), POISON, dtype=torch.float32, device="cuda")
        rec_b, ld_b, val_b = buffers()
        rec_c, ld_c, val_c = buffers()
        rec_d, ld_d, val_d = buffers()
        torch.cuda.synchronize()                                             # the fills (torch's stream) end before the handles' streams write
        ep = aforms.episode_buffers(T * n) if records_on else None
        run = dict(actions="actor", epsilon=eps, action_seed=seed, action_tick0=tick0)
        b.RolloutFusedDevice(None, T, episodes=ep, rec_logd=ld_b[:T], rec_value=val_b[:T], **run, **rec_b)
        c.RolloutFusedDevice(None, T, rec_logd=ld_c[:T], **run, **rec_c)
        spec = _spec(capi, T, capi.ACTIONS_ACTOR, eps, seed, tick0, d_rec_obs=rec_d["rec_obs"], d_rec_reward=rec_d["rec_reward"], d_rec_done=rec_d["rec_done"],
                     d_rec_actions=rec_d["rec_actions"])
        assert d._lib.gymnet_vecenv_rollout_fused_box_logd_device(d._h, C.byref(spec), None, C.c_void_p(val_d.data_ptr())) == capi.OK
        assert b.KernelName() == name0 == a.KernelName()                     # the handle's own step kernel is what the row's shape resolves to, before and after
        got_l, got_v = bits(host(ld_b)), bits(host(val_b))
        assert np.array_equal(got_l[:T], np.stack(logd_a)), np.argwhere(got_l[:T] != np.stack(logd_a))[:8]
        assert np.array_equal(got_v[:T], np.stack(value_a)), np.argwhere(got_v[:T] != np.stack(value_a))[:8]
        assert (host(ld_b)[T] == F32(POISON)).all() and (host(val_b)[T] == F32(POISON)).all()        # nothing past row T - 1
        assert np.array_equal(bits(host(ld_c)), got_l) and (host(val_c) == F32(POISON)).all()        # rec_logd alone
        assert np.array_equal(bits(host(val_d)), got_v) and (host(ld_d) == F32(POISON)).all()        # rec_value alone
        assert np.array_equal(bits(host(rec_b["rec_actions"])), bits(np.stack(act_a)))
        assert np.array_equal(bits(host(rec_b["rec_obs"])), bits(np.stack(obs_a)))
        assert np.array_equal(bits(host(rec_b["rec_reward"])), bits(np.stack(rew_a)))
        assert np.array_equal(host(rec_b["rec_done"]), np.stack(done_a))
        for other_rec in (rec_c, rec_d):                                     # the other streams are unchanged
            for k in rec_b:
                assert np.array_equal(host(other_rec[k]).view(np.uint8), host(rec_b[k]).view(np.uint8)), k
        for other in (b, c, d):
            assert np.array_equal(bits(a.GetState()), bits(other.GetState()))
            assert np.array_equal(a.GetArray("done"), other.GetArray("done"))
            assert a.Tick == other.Tick == tick_start + T
            if bookkeeping:
                for k in ("episode_return", "episode_length", "finished_return", "finished_length"):
                    assert np.array_equal(a.GetArray(k), other.GetArray(k)), k
            if not kw.get("auto_reset"):
                ca, co = a.Counters(), other.Counters()
                assert ca["stepped_after_done"] == co["stepped_after_done"] and ca["lane_steps"] == co["lane_steps"]
        for other in (actor_b, actor_c, actor_d):
            assert np.array_equal(actor_a.History(), other.History())
            assert other.Policy == (policy[0], policy[1], float(F32(policy[2])))
        if records_on:
            recs, kept, ended = aforms.records(ep)
            assert ended == len(want) and kept == ended and recs == sorted(want)
        assert np.array_equal(bits(host(actor_a.Value())), bits(host(actor_b.Value())))              # the last value, and the next decision
        nxt = bits(host(actor_a.Step(eps, seed, tick0 + T, logd=ld))).copy()
        nxt_l = bits(host(ld)).copy()
        assert np.array_equal(nxt, bits(host(actor_b.Step(eps, seed, tick0 + T, logd=ld)))) and np.array_equal(nxt_l, bits(host(ld)))
        return dict(actions=np.stack(act_a), logd=np.stack(logd_a), value=np.stack(value_a), done=np.stack(done_a))
    finally:
        for env in envs:
            env.Close()


@pytest.mark.parametrize("policy", forms.POLICIES, ids=lambda p: "-".join(map(str, p)))
@pytest.mark.parametrize("row", forms.FORMS, ids=forms.form_id)
def test_every_form_equals_single_steps(gpu_pkg, row, policy):
    """T = 12 with max_episode_steps = 5 on the bookkeeping rows, 3 warm steps so that the ring slot is not 0, MountainCarContinuous lanes
    put next to the goal: lanes restart inside the rollout, and truncate twice.  Under ("tanh", "gaussian", 0.3) with the [., 16, 1]
    critic, under ("clamp", "sample", 1.7) — the default pair, whose sigma only the log-density reads — with the [., 13, 7, 1] critic."""
    out = _fused_logd_equals_single_steps(gpu_pkg, row, policy)
    name = row["env"]
    low, high = box.BOUNDS[name]
    assert np.all((out["actions"] >= low) & (out["actions"] <= high))
    ld = out["logd"].view(F32)
    assert np.isfinite(ld).all() and (out["logd"] == _c_bits(policy[2])).any() and len(np.unique(out["logd"])) > N
    assert np.isfinite(out["value"].view(F32)).all() and len(np.unique(out["value"])) > N
    if row["shape"] != "lean":
        assert (out["done"] & 2).any()
        if row["auto_reset"]:
            assert (out["done"] & 2).sum(axis=0).max() >= 2                   # a lane truncates, restarts and truncates again
    if name == MCC:
        assert (out["done"][0][np.arange(N) % 3 == 0] & 1).all()


# ---- 3. the loop end to end ------------------------------------------------------------------------------------------------------------
def test_a_pendulum_rollout_feeds_the_advantages(gpu_pkg):
    """rec_value [T + 1, n] beside rec_logd: from the recorded observations and done bytes the history of every step is rebuilt on the
    host and the fmaf twin over the critic gives rec_value row by row, row T from the history after the rollout; the recorded logd is the
    twin's around the greedy action of the same rebuilt input; AdvantagesDevice over the device rows equals tests/_advantage_twin.py."""
    import torch
    eps, aseed, tick0, lane0, sigma = 1.0, 99, 1000, 7, 0.5
    critic = _critic(PENDULUM, True)
    with gpu_pkg.VectorEnv(PENDULUM, N, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=5, lane_offset=lane0) as env:
        obs0 = env.Reset()
        aw, aflat, apairs = _net(PENDULUM, twin.History(obs0, S).x())
        actor = env.Actor(apairs, history=S)
        actor.SetCritic(critic[2])
        actor.SetPolicy("clamp", "gaussian", sigma)
        rec = dict(rec_obs=torch.empty((T, env.ObsDim, N), dtype=torch.float32, device="cuda"), rec_done=torch.empty((T, N), dtype=torch.uint8, device="cuda"),
                   rec_reward=torch.empty((T, N), dtype=torch.float32, device="cuda"), rec_actions=torch.empty((T, N), dtype=torch.float32, device="cuda"),
                   rec_logd=torch.empty((T, N), dtype=torch.float32, device="cuda"), rec_value=torch.full((T + 1, N), POISON, dtype=torch.float32, device="cuda"))
        torch.cuda.synchronize()
        env.RolloutFusedDevice(None, T, actions="actor", epsilon=eps, action_seed=aseed, action_tick0=tick0, **rec)
        got = {k: host(v).copy() for k, v in rec.items()}
        model = twin.History(obs0, S)
        w, flat, _ = critic
        low, high = box.BOUNDS[PENDULUM]
        for t in range(T):
            want = twin.forward(w, flat, model.x())[0][:, 0]
            assert twin.same(got["rec_value"][t], want), (t, np.nonzero(got["rec_value"][t] != want)[0][:8])
            g = box.clamp(twin.forward(aw, aflat, model.x())[0][:, 0], low, high)          # the clamp head of the fmaf twin's output: exact
            want_ld = dtwin.logd(got["rec_actions"][t], g, sigma)
            assert np.array_equal(bits(got["rec_logd"][t]), bits(want_ld)), (t, np.nonzero(bits(got["rec_logd"][t]) != bits(want_ld))[0][:8])
            model.push(got["rec_obs"][t].T, got["rec_done"][t])
        assert np.array_equal(actor.History(), model.h)
        assert twin.same(got["rec_value"][T], twin.forward(w, flat, model.x())[0][:, 0])          # the last value
        assert (got["rec_done"] & 2).any() and len(np.unique(got["rec_value"].view(np.uint32))) > N
        assert len(np.unique(bits(got["rec_logd"]))) > T * N // 4
        adv, ret = (torch.empty((T, N), dtype=torch.float32, device="cuda") for _ in range(2))
        env.AdvantagesDevice(rec["rec_reward"], rec["rec_done"], rec["rec_value"], adv, ret, gamma=0.99, lam=0.95)
        want_adv, want_ret = atwin.gae(got["rec_reward"], got["rec_done"], got["rec_value"][:T], got["rec_value"][T], None, 0.99, 0.95)
        assert atwin.same(host(adv), want_adv) and atwin.same(host(ret), want_ret)
        assert np.isfinite(want_adv).all() and len(np.unique(want_adv)) > N


# ---- 4. refusals write nothing and leave the handle usable -----------------------------------------------------------------------------
def test_refusals_write_nothing(gpu_pkg):
    import importlib
    import torch
    capi = importlib.import_module(gpu_pkg.__name__ + "._capi")
    R = 4

    def buffers(n, adtype):
        b = dict(acts=torch.full((n,), -7, dtype=adtype, device="cuda"), logd=torch.full((n,), POISON, dtype=torch.float32, device="cuda"),
                 rec_logd=torch.full((R, n), POISON, dtype=torch.float32, device="cuda"), rec_value=torch.full((R, n), POISON, dtype=torch.float32, device="cuda"),
                 rec_act=torch.full((R, n), -7, dtype=adtype, device="cuda"))
        torch.cuda.synchronize()
        return b

    def intact(b):
        torch.cuda.synchronize()
        return all(bool((b[k] == (-7 if k in ("acts", "rec_act") else POISON)).all()) for k in b)

    def p(t, off=0):
        return C.c_void_p(t.data_ptr() + off)

    def act_logd(lib, h, b, eps=0.5, off=0):
        return lib.gymnet_vecenv_actor_box_act_logd_device(h, p(b["acts"]), None, p(b["logd"], off), C.c_float(eps), 5, 3)

    def fused(lib, h, b, source=None, logd=True, value=False, off=0, value_off=0, eps=0.5, steps=R):
        spec = _spec(capi, steps, capi.ACTIONS_ACTOR if source is None else source, eps, 99, 1000, d_rec_actions=b["rec_act"])
        return lib.gymnet_vecenv_rollout_fused_box_logd_device(h, C.byref(spec), p(b["rec_logd"], off) if logd else None,
                                                               p(b["rec_value"], value_off) if value else None)

    def unchanged(env, actor, state, tick, hist):
        env.Sync()
        return np.array_equal(bits(env.GetState()), bits(state)) and env.Tick == tick and np.array_equal(actor.History(), hist)

    # a Discrete actor, float32 and float64: both new calls refuse it
    for kw in ({}, dict(dtype=np.float64)):
        with gpu_pkg.VectorEnv("CartPole-v1", N, seed=SEED, auto_reset=True, **kw) as env:
            env.Reset()
            lib, h = env._lib, env._h
            b = buffers(N, torch.int32)
            assert act_logd(lib, h, b) == capi.ERR_INVALID_ARG and b"gymnet_vecenv_actor_box_config" not in lib.gymnet_last_error()      # no actor
            actor = env.Actor(twin.net(np.random.default_rng(2), [4, 2])[2], 1)
            before = host(actor.Act(0.3, 5, 3)).copy()
            assert act_logd(lib, h, b) == capi.ERR_INVALID_ARG and b"gymnet_vecenv_actor_act_logp_device" in lib.gymnet_last_error()
            assert fused(lib, h, b) == capi.ERR_INVALID_ARG and b"Discrete" in lib.gymnet_last_error()
            assert fused(lib, h, b, logd=False, value=True) == capi.ERR_INVALID_ARG and b"Discrete" in lib.gymnet_last_error()
            logd = torch.empty(N, dtype=torch.float32, device="cuda")
            with pytest.raises(ValueError, match="Discrete"):
                actor.Act(0.3, 5, 3, logd=logd)
            with pytest.raises(ValueError, match="Discrete"):
                env.RolloutFusedDevice(None, R, actions="actor", rec_logd=b["rec_logd"])
            assert intact(b)
            assert np.array_equal(host(actor.Act(0.3, 5, 3)), before)
            actor.Step(0.3, 5, 3)
    with gpu_pkg.VectorEnv(PENDULUM, N, seed=SEED) as env:
        env.Reset()
        lib, h = env._lib, env._h
        b = buffers(N, torch.float32)
        assert act_logd(lib, h, b) == capi.ERR_INVALID_ARG and b"gymnet_vecenv_actor_box_config" in lib.gymnet_last_error()              # no actor
        assert fused(lib, h, b) == capi.ERR_INVALID_ARG and b"gymnet_vecenv_actor_box_config" in lib.gymnet_last_error()
        actor = env.Actor(_net(PENDULUM)[2], history=S)
        state, tick, hist = env.GetState(), env.Tick, actor.History()

        def refused(status=capi.ERR_INVALID_ARG, word=None, policy=None, **kw):
            got = fused(lib, h, b, **kw)
            assert got == status, (kw, got, lib.gymnet_last_error())
            assert word is None or word in lib.gymnet_last_error(), lib.gymnet_last_error()
            assert intact(b) and unchanged(env, actor, state, tick, hist)
            assert policy is None or actor.Policy == policy

        # sigma = 0, the fresh default
        assert act_logd(lib, h, b) == capi.ERR_INVALID_ARG and b"sigma" in lib.gymnet_last_error()
        refused(word=b"sigma", policy=("clamp", "sample", 0.0))
        with pytest.raises(ValueError, match="sigma"):                     # (the library's refusal: the wrapper does not read the policy)
            actor.Act(0.3, 5, 3, logd=b["logd"])
        # a sigma so small that 1 / sigma overflows: set_policy stores it, the request refuses it
        tiny = float(np.float32(1e-39))
        actor.SetPolicy("tanh", "gaussian", tiny)
        assert act_logd(lib, h, b) == capi.ERR_INVALID_ARG and b"sigma" in lib.gymnet_last_error()
        refused(word=b"sigma", policy=("tanh", "gaussian", tiny))
        refused(word=b"sigma", logd=False, value=True)
        actor.Step(0.3, 5, 3)                                                 # the plain calls serve such a policy as before
        state, tick, hist = env.GetState(), env.Tick, actor.History()
        actor.SetPolicy("tanh", "gaussian", 0.5)
        # rec_value without a critic; logd alone needs none
        refused(word=b"critic", value=True)
        refused(word=b"critic", logd=False, value=True)
        with pytest.raises(ValueError, match="critic"):
            env.RolloutFusedDevice(None, R, actions="actor", rec_logd=b["rec_logd"], rec_value=b["rec_value"])
        critic = _critic(PENDULUM, False)
        actor.SetCritic(critic[2])
        with pytest.raises(ValueError, match="Box"):                          # rec_value alone keeps raising in Python
            env.RolloutFusedDevice(None, R, actions="actor", rec_value=b["rec_value"])
        # misaligned pointers, other sources, the rollout's own checks, the act call's
        refused(word=b"d_rec_logd must be 4-byte aligned", off=2)
        refused(word=b"d_rec_value must be 4-byte aligned", value=True, value_off=2)
        refused(word=b"d_rec_logd must be 4-byte aligned", value=True, off=1, value_off=2)
        for source in (capi.ACTIONS_RING, capi.ACTIONS_SAMPLE, capi.ACTIONS_EPSILON_GREEDY, 7):
            refused(word=b"GYMNET_ACTIONS_ACTOR", source=source)
        refused(word=b"epsilon", eps=1.5)
        assert lib.gymnet_vecenv_rollout_fused_box_logd_device(h, None, p(b["rec_logd"]), None) == capi.ERR_INVALID_ARG                  # a null spec
        assert act_logd(lib, h, b, off=2) == capi.ERR_INVALID_ARG and b"d_logd" in lib.gymnet_last_error()
        assert act_logd(lib, h, b, eps=1.5) == capi.ERR_INVALID_ARG
        assert lib.gymnet_vecenv_actor_box_act_logd_device(h, None, None, p(b["logd"]), C.c_float(0.5), 5, 3) == capi.ERR_INVALID_ARG
        assert fused(lib, h, b, value=True, steps=0) == capi.OK               # steps == 0 writes nothing and is no error
        assert intact(b) and unchanged(env, actor, state, tick, hist) and actor.Policy == ("tanh", "gaussian", 0.5)
        # a stale history: one step without a push
        env.StepDevice(actor.Act(0.5, 5, 3))
        state, tick = env.GetState(), env.Tick
        assert act_logd(lib, h, b) == capi.ERR_INVALID_ARG and b"stale" in lib.gymnet_last_error()
        refused(word=b"stale", value=True)
        actor.Push()                                                          # ... and after the push both serve again
        assert act_logd(lib, h, b) == capi.OK and fused(lib, h, b, value=True) == capi.OK
        env.Sync()
        assert not any(bool((b[k] == POISON).any()) for k in ("logd", "rec_logd", "rec_value"))
        # the pointers belong to the one call that was given them: a plain rollout after it leaves them alone
        b = buffers(N, torch.float32)
        env.RolloutFusedDevice(None, R, actions="actor", epsilon=0.5, rec_actions=b["rec_act"])
        env.Sync()
        assert bool((b["rec_logd"] == POISON).all()) and bool((b["rec_value"] == POISON).all()) and not bool((b["rec_act"] == -7).any())
        # SetPolicy between two calls changes c from the next launch on
        for sigma in (0.5, 1.7, 0.25):
            actor.SetPolicy("tanh", "gaussian", sigma)
            assert act_logd(lib, h, b, eps=0.0) == capi.OK
            assert (bits(host(b["logd"])) == _c_bits(sigma)).all(), sigma
            assert fused(lib, h, b, eps=0.0) == capi.OK
            assert (bits(host(b["rec_logd"])) == _c_bits(sigma)).all(), sigma
        assert twin.same(host(actor.Value()), _want_value(critic, actor))
        actor.Step(0.5, 5, 3)
