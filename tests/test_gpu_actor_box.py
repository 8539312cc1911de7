"""GPU checks of the Box actor (gym.net_amd/csrc/actor_box.hip, gymnet_vecenv_actor_box_*) on Pendulum and MountainCarContinuous: the
unclamped outputs bit-identical to the fmaf twin (tests/_actor_twin.py, -0 == +0) and the actions equal to where(explore, sample,
clamp(raw)) with the oracle's words, on weights rescaled so that the clamp works on both sides; every one of the 12 fused rollout
forms (tests/_actor_box_forms.py) against T single closed-loop steps; the fused rollout replayed on the CPU; 64-bit action ticks and
seeds, and shards whose boundary crosses a group of four lanes; refusals that write nothing; an EpisodeMemory fed by the actor."""
import ctypes as C

import numpy as np
import pytest

import _actor_box_forms as box
import _actor_forms as forms
import _actor_twin as twin
import _mountaincar_continuous_twin as mcc

pytestmark = pytest.mark.gpu
SEED = 0xAC7
F32 = np.float32
PENDULUM, MCC = "Pendulum-v1", "MountainCarContinuous-v0"
ACT_CASES = [(PENDULUM, [3, 1], 1), (PENDULUM, [12, 50, 20, 1], 4), (PENDULUM, [63, 64, 33, 1], 21), (MCC, [64, 4, 8, 1], 32)]
HIDDEN = {PENDULUM: [50, 20], MCC: [13, 7]}
host = forms.host


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _rescaled(rng, widths, x0, low, high):
    """A random network whose output layer is shifted and scaled, from the twin's numbers over the inputs x0: the output bias moves by
    the median of raw, then the output row and bias are scaled about it so that the quartiles land on `low` and `high` (the bounds are
    symmetric): about a quarter of the lanes clamps on either side.  Returns (widths, flat, pairs)."""
    w, flat, _ = twin.net(rng, widths)
    raw = twin.forward(w, flat, x0)[0][:, 0].astype(np.float64)
    q25, med, q75 = np.percentile(raw, [25, 50, 75])
    flat = flat.copy()
    last = widths[-2] + 1                                   # the output row and its bias are the block's tail
    flat[-1] = F32(flat[-1] - med)
    if q75 > q25:                                           # (one lane: nothing to scale)
        flat[-last:] = (flat[-last:] * F32((high - low) / (q75 - q25))).astype(F32)
        flat[-1] = F32(flat[-1] + (low + high) / 2 - (high - low) * ((q25 + q75) / 2 - med) / (q75 - q25))   # the quartiles' midpoint to the bounds'
    return w, flat, twin.layers(widths, flat)


def _words(oracle, seed, lane0, tick, n):
    return oracle.action_words(int(seed), int(lane0), int(tick), n)


@pytest.mark.parametrize("n", [1, 63, 65, 257, 1000])
@pytest.mark.parametrize("name,widths,S", ACT_CASES)
def test_raw_and_actions_equal_the_twin(gpu_pkg, oracle, name, widths, S, n):
    import torch
    rng = np.random.default_rng(n + S)
    low, high = box.BOUNDS[name]
    with gpu_pkg.VectorEnv(name, n, seed=SEED, auto_reset=True) as env:
        obs = env.Reset()
        x0 = twin.History(obs, S).x()
        w, flat, pairs = _rescaled(rng, widths, x0, low, high)
        raw0 = twin.forward(w, flat, x0)[0][:, 0]
        if n == 1000:                                        # the inputs exercise the clamp on both sides: from the twin's numbers
            assert (raw0 < low).mean() >= 0.2 and (raw0 > high).mean() >= 0.2 and ((raw0 > low) & (raw0 < high)).mean() >= 0.2
        actor = env.Actor(pairs, history=S)
        assert actor.IsBox
        raw = torch.empty((n, 1), dtype=torch.float32, device="cuda")
        tick = 12
        for step in range(3):                                # at the initial histories, then after closed-loop steps (ring slots 1, 2)
            x = actor.History().reshape(n, -1)
            want_raw = twin.forward(w, flat, x)[0]
            if step == 0:
                assert np.array_equal(x, x0)
            for eps in (0.0, 0.3, 1.0):
                raw.fill_(-7.0)
                torch.cuda.synchronize()                                     # the fill (torch's stream) ends before the handle's stream writes
                got = actor.Act(eps, seed=77, tick=tick, logits=raw)
                assert got.dtype == torch.float32 and tuple(got.shape) == (n,)
                assert twin.same(host(raw), want_raw)
                wa, wb = _words(oracle, 77, 0, tick, n)
                want, explore = box.compose(want_raw[:, 0], wa, wb, eps, low, high)
                assert np.array_equal(box.sample(wa, low, high), oracle.box_uniform_sample(77, 0, tick, low, high, n))
                if name == MCC:
                    assert np.array_equal(box.sample(wa, low, high), mcc.box_sample(77, 0, tick, n))
                assert twin.same(host(got), want)
                assert np.array_equal(host(got)[explore].view(np.uint32), want[explore].view(np.uint32))
                if eps == 0.0:
                    assert not explore.any()
                if eps == 1.0:
                    assert explore.all()
                if eps == 0.3 and n == 1000:
                    assert explore.mean() >= 0.2 and (~explore).mean() >= 0.5
            tick += 1
            actor.Step(0.3, 78, tick)


def test_a_nan_output_bias_passes_the_clamp_and_leaves_the_samples(gpu_pkg, oracle):
    n, S = 1000, 4
    rng = np.random.default_rng(9)
    with gpu_pkg.VectorEnv(PENDULUM, n, seed=SEED) as env:
        env.Reset()
        w, flat, _ = twin.net(rng, [12, 50, 20, 1])
        flat[-1] = np.nan
        actor = env.Actor(twin.layers([12, 50, 20, 1], flat), history=S)
        got = host(actor.Act(0.3, seed=5, tick=3))
        wa, wb = _words(oracle, 5, 0, 3, n)
        explore = wb <= np.uint32(box.coin_threshold(0.3))
        assert explore.any() and (~explore).any()
        assert np.isnan(got[~explore]).all()
        assert np.array_equal(got[explore].view(np.uint32), box.sample(wa, -2.0, 2.0)[explore].view(np.uint32))


def _near_goal(lane_offset=0, second=False):
    """every third (global) lane one step from the goal: position just below GOAL, velocity 0.03; second: the lanes after them two steps
    from it (position 0.40: 0.4276 .. 0.4306 after one step whatever the force, past 0.45 after two)"""
    def prepare(env):
        s = env.GetState()
        k = (np.arange(env.NumberOfEnvironments) + lane_offset) % 3
        s[0, k == 0], s[1, k == 0] = mcc.BELOW_GOAL32, F32(0.03)
        if second:
            s[0, k == 1], s[1, k == 1] = F32(0.40), F32(0.03)
        env.SetState(s)
    return prepare


def _net_for(name, S, seed=1):
    O = 3 if name == PENDULUM else 2
    widths = [S * O] + HIDDEN[name] + [1]
    return twin.net(np.random.default_rng(seed), widths, scale=4.0)


@pytest.mark.parametrize("row", box.FORMS, ids=box.form_id)
def test_every_form_equals_single_steps(gpu_pkg, row):
    n, T, S = 1000, 40, 4
    name, bookkeeping = row["env"], row["shape"] != "lean"
    w, flat, pairs = _net_for(name, S)
    kw = forms.handle_kwargs(row)
    third = np.arange(n) % 3 == 0

    def masked_reset(env, actor):
        m = _dev(third.astype(np.uint8))
        env.ResetWhereDevice(m)
        actor.Reset(m)

    def near_goal(env, actor):                               # after the warm steps, so that the rollout starts from a ring slot other than 0
        _near_goal(second=True)(env)
        actor.Reset()
    pendulum_book = name == PENDULUM and bookkeeping
    out = box.fused_equals_single_steps(gpu_pkg, name, n, T, kw, row["shape"] == "records", pairs, S=S, warm=7 if pendulum_book else 3,
                                        after_warm=near_goal if name == MCC else masked_reset if pendulum_book else None)
    done = out["done"]
    first = np.where(done.any(axis=0), np.argmax(done != 0, axis=0), -1)      # the step each lane's first episode ends on
    if name == MCC:
        assert (done[0][third] & 1).all()                                  # the prepared lanes reach the goal in step 0,
        assert (first[np.arange(n) % 3 == 1] == 1).all()                   # their neighbours in step 1
        if bookkeeping:
            assert (first[~third] > 0).all() and (done[21][~third] & 2).any()   # and the time limit takes lanes that did not: 25 - 3 warm steps
    if pendulum_book:
        # the time limit: 25 - 7 warm steps for the lanes that kept their episode, 25 for the lanes the masked reset restarted
        assert (first[~third] == 17).all() and (done[17][~third] == 2).all()
        assert (first[third] == 24).all() and (done[24][third] == 2).all()
    if bookkeeping or name == MCC:
        assert len(set(first[first >= 0].tolist())) > 1


def _replay_actions(oracle, w, flat, hist, eps, seed, lane0, tick, low, high):
    raw = twin.forward(w, flat, hist.x())[0][:, 0]
    wa, wb = _words(oracle, seed, lane0, tick, len(raw))
    act, explore = box.compose(raw, wa, wb, eps, low, high)
    return act, int(((raw < low) | (raw > high))[~explore].sum())      # and how many greedy actions the clamp changed


def _fused(env, T, eps, seed, tick0):
    import torch
    n, O = env.NumberOfEnvironments, env.ObsDim
    rec = dict(rec_obs=torch.empty((T, O, n), dtype=torch.float32, device="cuda"), rec_reward=torch.empty((T, n), dtype=torch.float32, device="cuda"),
               rec_done=torch.empty((T, n), dtype=torch.uint8, device="cuda"), rec_actions=torch.empty((T, n), dtype=torch.float32, device="cuda"))
    env.RolloutFusedDevice(None, T, actions="actor", epsilon=eps, action_seed=seed, action_tick0=tick0, **rec)
    return {k: host(v) for k, v in rec.items()}


def test_mountaincar_continuous_rollout_equals_the_cpu_replay(gpu_pkg, oracle):
    n, T, S, eps, aseed, atick0 = 257, 12, 4, 0.3, 99, 1000
    w, flat, pairs = _net_for(MCC, S)
    with gpu_pkg.VectorEnv(MCC, n, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=5) as env:
        env.Reset()
        _near_goal()(env)
        actor = env.Actor(pairs, S)
        tick0 = env.Tick
        rp = mcc.Replay(env.GetState(), SEED, 0, True, True, 5)
        hist = twin.History(env.GetState().T, S)
        assert np.array_equal(actor.History(), hist.h)
        got = _fused(env, T, eps, aseed, atick0)
        clamped = 0
        for t in range(T):
            a, c = _replay_actions(oracle, w, flat, hist, eps, aseed, 0, atick0 + t, -1.0, 1.0)
            clamped += c
            assert np.array_equal(got["rec_actions"][t].view(np.uint32), a.view(np.uint32)), t
            obs, rw, db, fin = rp.step(a, tick0 + t)
            assert np.array_equal(box.bits(got["rec_obs"][t]), box.bits(obs)), t
            assert np.array_equal(box.bits(got["rec_reward"][t]), box.bits(rw)) and np.array_equal(got["rec_done"][t], db), t
            if t == 0:
                assert fin[np.arange(n) % 3 == 0].all()
            hist.push(obs.T, db)
        assert (got["rec_done"] & 2).any() and np.array_equal(actor.History(), hist.h)
        assert clamped > 0


def _pendulum_replay(oracle, env, actor, w, flat, S, T, eps, aseed, atick0, lane0=0):
    """the fused rollout of a Pendulum handle without a time limit against oracle.env_step in float32"""
    state = env.GetState()
    hist = twin.History(env.Read().Observation, S)
    assert np.array_equal(actor.History(), hist.h)
    got = _fused(env, T, eps, aseed, atick0)
    clamped = 0
    for t in range(T):
        a, c = _replay_actions(oracle, w, flat, hist, eps, aseed, lane0, atick0 + t, -2.0, 2.0)
        clamped += c
        assert np.array_equal(got["rec_actions"][t].view(np.uint32), a.view(np.uint32)), t
        state, obs, rw, dn = oracle.env_step(PENDULUM, state, a, dtype=np.float32)
        assert np.array_equal(box.bits(got["rec_obs"][t]), box.bits(obs)), t
        assert np.array_equal(box.bits(got["rec_reward"][t]), box.bits(rw)) and np.array_equal(got["rec_done"][t], dn), t
        hist.push(obs.T, dn)
    assert np.array_equal(box.bits(env.GetState()), box.bits(state)) and np.array_equal(actor.History(), hist.h)
    assert clamped > 0
    return got


def test_pendulum_rollout_equals_the_cpu_replay(gpu_pkg, oracle):
    n, S = 257, 4
    w, flat, pairs = _net_for(PENDULUM, S)
    with gpu_pkg.VectorEnv(PENDULUM, n, seed=SEED) as env:
        env.Reset()
        actor = env.Actor(pairs, S)
        _pendulum_replay(oracle, env, actor, w, flat, S, 12, 0.3, 99, 1000)


def test_action_ticks_and_seeds_beyond_32_bits(gpu_pkg, oracle):
    n, S, T, eps = 257, 4, 6, 0.3
    aseed, atick0 = 0x1_0000_0063, 2 ** 32 - 2
    w, flat, pairs = _net_for(PENDULUM, S)
    out = box.fused_equals_single_steps(gpu_pkg, PENDULUM, n, T, dict(auto_reset=False), False, pairs, S=S, eps=eps, seed=aseed, tick0=atick0)
    with gpu_pkg.VectorEnv(PENDULUM, n, seed=SEED) as env:                    # the same env seed as the comparison's handles
        env.Reset()
        actor = env.Actor(pairs, S)
        got = _pendulum_replay(oracle, env, actor, w, flat, S, T, eps, aseed, atick0)
    assert np.array_equal(box.bits(got["rec_actions"]), box.bits(out["actions"]))
    # the high halves matter: the low 32 bits alone draw other words
    wa_low, _ = _words(oracle, aseed & 0xFFFFFFFF, 0, (atick0 + 2) & 0xFFFFFFFF, n)
    assert not np.array_equal(wa_low, _words(oracle, aseed, 0, atick0 + 2, n)[0])


def test_shards_whose_boundary_crosses_a_group_of_four(gpu_pkg):
    S, T, eps = 4, 8, 0.3
    w, flat, pairs = _net_for(MCC, S)

    def run(n, lane0, state):
        with gpu_pkg.VectorEnv(MCC, n, seed=SEED, auto_reset=True, lane_offset=lane0) as env:
            env.Reset()
            if state is not None:
                env.SetState(state)
            _near_goal(lane0)(env)
            s0 = env.GetState()
            env.Actor(pairs, S)
            return s0, _fused(env, T, eps, 99, 1000)
    s0, whole = run(2048, 0, None)
    assert 1001 % 4 != 0
    parts = [run(1001, 0, s0[:, :1001])[1], run(1047, 1001, s0[:, 1001:])[1]]
    for k in ("rec_actions", "rec_obs", "rec_done"):
        joined = np.concatenate([p[k] for p in parts], axis=-1)
        assert np.array_equal(joined.view(np.uint8), whole[k].view(np.uint8)), k
    assert whole["rec_done"].any()


def test_refusals_write_nothing(gpu_pkg):
    import importlib
    import torch
    capi = importlib.import_module(gpu_pkg.__name__ + "._capi")
    n = 256

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p)

    def box_net(widths):
        w, flat, pairs = twin.net(np.random.default_rng(2), widths)
        return w, flat, pairs
    poison_f = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    poison_i = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True) as env:         # a Discrete env
        env.Reset()
        lib, h = env._lib, env._h
        w, flat, pairs = box_net([4, 1])
        assert lib.gymnet_vecenv_actor_box_config(h, 1, 1, ptr(w), ptr(flat), flat.size) == capi.ERR_UNSUPPORTED
        assert lib.gymnet_vecenv_actor_box_act_device(h, C.c_void_p(poison_f.data_ptr()), None, 0.0, 0, 0) == capi.ERR_INVALID_ARG   # no actor
        env.Actor(twin.net(np.random.default_rng(2), [4, 2])[2], 1)
        assert lib.gymnet_vecenv_actor_box_act_device(h, C.c_void_p(poison_f.data_ptr()), None, 0.0, 0, 0) == capi.ERR_INVALID_ARG   # a Discrete one
        assert b"gymnet_vecenv_actor_act_device" in lib.gymnet_last_error()
        assert bool((poison_f == -7.0).all())
    with gpu_pkg.VectorEnv(PENDULUM, n, seed=SEED) as env:
        env.Reset()
        lib, h = env._lib, env._h
        w, flat, pairs = box_net([3, 1])
        assert lib.gymnet_vecenv_actor_config(h, 1, 1, ptr(w), ptr(flat), flat.size) == capi.ERR_UNSUPPORTED
        assert b"gymnet_vecenv_actor_box_config" in lib.gymnet_last_error()
        # a fused actor rollout with no actor configured
        rec = torch.full((4, n), -7.0, dtype=torch.float32, device="cuda")
        spec = capi.RolloutSpec(struct_size=C.sizeof(capi.RolloutSpec), action_source=capi.ACTIONS_ACTOR, steps=4, d_rec_actions=rec.data_ptr(),
                                d_rec_reward=rec.data_ptr())
        tick = env.Tick
        assert lib.gymnet_vecenv_rollout_fused_ex_device(h, C.byref(spec)) == capi.ERR_INVALID_ARG
        assert env.Tick == tick and bool((rec == -7.0).all())
        w2, flat2, _ = box_net([3, 2])                                                   # a last width of 2
        assert lib.gymnet_vecenv_actor_box_config(h, 1, 1, ptr(w2), ptr(flat2), flat2.size) == capi.ERR_INVALID_ARG
        with pytest.raises(ValueError):
            env.Actor(twin.layers([3, 2], flat2), 1)
        w22, flat22, _ = box_net([66, 1])                                                # a history of 22: 66 inputs
        assert lib.gymnet_vecenv_actor_box_config(h, 22, 1, ptr(w22), ptr(flat22), flat22.size) == capi.ERR_INVALID_ARG
        assert lib.gymnet_vecenv_actor_box_act_device(h, C.c_void_p(poison_f.data_ptr()), None, 0.0, 0, 0) == capi.ERR_INVALID_ARG   # still no actor
        assert lib.gymnet_vecenv_actor_act_device(h, C.c_void_p(poison_i.data_ptr()), None, 0.0, 0, 0) == capi.ERR_INVALID_ARG
        assert b"gymnet_vecenv_actor_box_config" in lib.gymnet_last_error()
        actor = env.Actor(pairs, 1)
        assert actor.History().shape == (n, 1, 3)
        assert lib.gymnet_vecenv_actor_act_device(h, C.c_void_p(poison_i.data_ptr()), None, 0.0, 0, 0) == capi.ERR_INVALID_ARG       # the other kind
        assert b"gymnet_vecenv_actor_box_act_device" in lib.gymnet_last_error()
        assert bool((poison_i == -7).all())
        assert lib.gymnet_vecenv_actor_box_act_device(h, C.c_void_p(poison_f.data_ptr()), None, 1.5, 0, 0) == capi.ERR_INVALID_ARG   # epsilon
        assert lib.gymnet_vecenv_actor_box_act_device(h, None, None, 0.0, 0, 0) == capi.ERR_INVALID_ARG                              # null
        env.StepDevice(_dev(np.zeros(n, F32)))                                           # a plain step: the history is stale
        assert lib.gymnet_vecenv_actor_box_act_device(h, C.c_void_p(poison_f.data_ptr()), None, 0.0, 0, 0) == capi.ERR_INVALID_ARG
        assert lib.gymnet_vecenv_rollout_fused_ex_device(h, C.byref(spec)) == capi.ERR_INVALID_ARG
        assert bool((poison_f == -7.0).all()) and bool((rec == -7.0).all())
        actor.Push()
        assert host(actor.Act()).dtype == np.float32
        # a history of 21 is the widest Pendulum takes
        w21, flat21, pairs21 = box_net([63, 1])
        assert env.Actor(pairs21, 21).History().shape == (n, 21, 3)


def test_an_episode_memory_keeps_the_actions_the_actor_returned(gpu_pkg):
    import _episode_memory_model as model
    n, S, steps = 64, 4, 30
    w, flat, pairs = _net_for(PENDULUM, S)
    with gpu_pkg.VectorEnv(PENDULUM, n, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=10) as env:
        obs = env.Reset()
        actor = env.Actor(pairs, S)
        mem = env.EpisodeMemory(capacity=8, history=4)
        m = model.EpisodeMemoryModel(obs, 8, 10, 4)
        for t in range(steps):
            taken = actor.Step(0.3, 99, 1000 + t)
            a = host(taken).copy()
            mem.Push(taken)
            r = env.Read()
            m.push(a, r.Reward, env.GetArray("done"), r.Observation, env.Tick)
        x, want_a, _, _ = m.dataset_params(None)
        assert len(m.pool) == 8 and len(want_a) == 8 * 6
        got = mem.BuildDataset("params", min_episodes=0)
        assert np.array_equal(host(got[1]).view(np.uint32), want_a.astype(F32).view(np.uint32))
        assert np.array_equal(host(got[0]), x)
