"""GPU checks of the actor (gym.net_amd/csrc/actor.hip, gymnet_vecenv_actor_*): logits and greedy actions bit-identical to the fmaf twin
(tests/_actor_twin.py, -0 == +0) on CartPole / MountainCar / Acrobot float32 and CartPole float64 handles; epsilon-greedy actions equal
to ComposeActionsDevice over the twin's greedy actions; the history against the NumPy model of its rules, with the handle's done bytes and
with the caller's own; the fused rollout (the comparison is tests/_actor_forms.py fused_equals_single_steps) with
GYMNET_ACTIONS_ACTOR bit-identical to steps x (Act, StepDevice, Push) on plain, trainer-shaped and done-list / terminal-observation
handles, episode records with their returns and lengths included; a closed loop against the oracle's step and Philox streams; params datasets of an
EpisodeMemory whose rows the twin maps to the actions taken; refusals that write nothing; Load.  The fused rollout's 18 kernel forms, its
record staging, the depth, shape, 2^32 and lane-offset edges are in tests/test_gpu_actor_forms.py."""
import ctypes as C

import numpy as np
import pytest

import _actor_forms as forms
import _actor_twin as twin

pytestmark = pytest.mark.gpu
SEED = 0xAC7
RUNNER = {"CartPole-v1": [16, 50, 20, 2], "MountainCar-v0": [8, 13, 7, 3], "Acrobot-v1": [24, 50, 20, 3]}


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


_net = twin.net


def _warm(env, actor, steps, rng):
    """a few random steps with pushes, so the histories differ from slot to slot"""
    n = env.NumberOfEnvironments
    for t in range(steps):
        env.StepDevice(_dev(rng.integers(0, env.ActionSpace.N, n).astype(np.int32)))
        actor.Push()


_same = twin.same


CASES = [("CartPole-v1", np.float32, 4, "runner", 1000), ("CartPole-v1", np.float32, 4, "runner", 1 << 20),
         ("CartPole-v1", np.float32, 1, "linear", 1000), ("CartPole-v1", np.float64, 4, "runner", 1000),
         ("CartPole-v1", np.float64, 1, "runner", 1 << 20), ("MountainCar-v0", np.float32, 4, "runner", 1000),
         ("MountainCar-v0", np.float32, 1, "linear", 1 << 20), ("Acrobot-v1", np.float32, 4, "runner", 1000),
         ("Acrobot-v1", np.float32, 1, "runner", 1 << 20), ("Acrobot-v1", np.float32, 4, "linear", 1000)]


@pytest.mark.parametrize("name,dtype,S,shape,n", CASES)
def test_logits_and_greedy_equal_the_twin(gpu_pkg, name, dtype, S, shape, n):
    import torch
    rng = np.random.default_rng(n + S)
    with gpu_pkg.VectorEnv(name, n, seed=SEED, auto_reset=True, dtype=dtype) as env:
        env.Reset()
        O, A = env.ObsDim, env.ActionSpace.N
        widths = [S * O] + RUNNER[name][1:-1] + [A] if shape == "runner" else [S * O, A]
        w, flat, pairs = _net(rng, widths)
        actor = env.Actor(pairs, history=S)
        _warm(env, actor, 5, rng)
        logits = torch.empty((n, A), dtype=torch.float32, device="cuda")
        act = actor.Act(logits=logits)
        x = actor.History().reshape(n, -1)
        want_l, want_g = twin.forward(w, flat, x)
        assert _same(_host(logits), want_l)
        assert np.array_equal(_host(act), want_g)


@pytest.mark.parametrize("eps", [0.0, 0.3, 1.0])
def test_epsilon_greedy_equals_compose(gpu_pkg, eps):
    import torch
    n = 4099
    rng = np.random.default_rng(3)
    with gpu_pkg.VectorEnv("MountainCar-v0", n, seed=SEED, auto_reset=True) as env:
        env.Reset()
        w, flat, pairs = _net(rng, [8, 13, 7, 3])
        actor = env.Actor(pairs, history=4)
        _warm(env, actor, 3, rng)
        _, greedy = twin.forward(w, flat, actor.History().reshape(n, -1))
        got = actor.Act(eps, seed=77, tick=12)
        want = torch.empty(n, dtype=torch.int32, device="cuda")
        env.ComposeActionsDevice(_dev(greedy), eps, want, seed=77, tick=12)
        assert np.array_equal(_host(got), _host(want))
        if eps == 0.0:
            assert np.array_equal(_host(got), greedy)


def _history_loop(gpu_pkg, auto_reset, own_done=0.0):
    """own_done: Push gets the caller's done bytes — the handle's OR a host-chosen mask of that density — and so does the model"""
    n, S = 2000, 3
    rng = np.random.default_rng(5)
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=auto_reset) as env:
        obs = env.Reset()
        w, flat, pairs = _net(rng, [S * 4, 20, 2])
        actor = env.Actor(pairs, history=S)
        model = twin.History(obs, S)
        assert np.array_equal(actor.History(), model.h)
        for t in range(40):
            out = env.Step(rng.integers(0, 2, n).astype(np.int32))
            d = out.Done.astype(np.uint8)
            if own_done:
                d |= (rng.random(n) < own_done).astype(np.uint8)
                actor.Push(_dev(d))
            else:
                actor.Push()
            model.push(out.Observation, d)
            if not auto_reset and d.any():
                obs = env.ResetWhere(d)
                actor.Reset(_dev(d))
                model.reset(obs, d)
            assert np.array_equal(actor.History(), model.h), t


@pytest.mark.parametrize("auto_reset", [True, False])
def test_history_follows_the_rules(gpu_pkg, auto_reset):
    _history_loop(gpu_pkg, auto_reset)


@pytest.mark.parametrize("auto_reset", [True, False])
def test_history_follows_the_rules_with_the_callers_done_bytes(gpu_pkg, auto_reset):
    _history_loop(gpu_pkg, auto_reset, own_done=0.05)


@pytest.mark.parametrize("name", ["CartPole-v1", "MountainCar-v0", "Acrobot-v1"])
@pytest.mark.parametrize("T", [1, 7, 64])
@pytest.mark.parametrize("trainer", [False, True, "full"])
def test_fused_actor_rollout_equals_single_steps(gpu_pkg, name, T, trainer, n=3000):
    """the comparison itself is tests/_actor_forms.py fused_equals_single_steps, shared with tests/test_gpu_actor_forms.py"""
    rng = np.random.default_rng(T)
    kw = dict(auto_reset=True)
    if trainer:
        kw.update(episode_stats=True, max_episode_steps=50)
    if trainer == "full":
        kw.update(done_list=True, final_obs=True)
    w, flat, pairs = _net(rng, RUNNER[name])                              # history 4: RUNNER's first width is 4 * obs_dim
    forms.fused_equals_single_steps(gpu_pkg, name, n, T, kw, bool(trainer), pairs, S=4, eps=0.3, seed=99, tick0=1000, full=trainer == "full",
                                    env_seed=SEED)


def test_closed_loop_matches_the_oracle(gpu_pkg, oracle):
    """4096 CartPole lanes, 200 closed-loop steps at epsilon 0.3: the oracle's float32 step and Philox resets, driven by the twin's greedy
    actions over a NumPy history and the epsilon composition rebuilt from the oracle's action-stream words, give the engine's actions,
    observations, rewards and dones after every actor.Step, bit for bit."""
    n, S, steps, eps, aseed = 4096, 4, 200, 0.3, 0xE95
    rng = np.random.default_rng(19)
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True) as env:
        first = env.Reset()
        s = oracle.cartpole_reset(SEED, 0, 0, n)
        assert np.array_equal(first.T, s)
        w, flat, pairs = _net(rng, RUNNER["CartPole-v1"])
        actor = env.Actor(pairs, history=S)
        model = twin.History(first, S)
        ended = explored = 0
        for t in range(steps):
            tick = env.Tick
            _, greedy = twin.forward(w, flat, model.x())
            wa, wb = oracle.action_words(aseed, 0, t, n)
            explore = ((wb >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)) <= np.float32(eps)   # NextDouble() <= epsilon
            sampled = ((wa.astype(np.uint64) * np.uint64(2)) >> np.uint64(32)).astype(np.int32)                       # ActionSpace.Sample()
            want_a = np.where(explore, sampled, greedy).astype(np.int32)
            assert np.array_equal(want_a, oracle.compose_discrete(aseed, 0, t, 2, eps, greedy))
            got_a = _host(actor.Step(eps, aseed, t))
            assert np.array_equal(got_a, want_a), t
            s, r, d, _ = oracle.cartpole_step(s, want_a, dtype=np.float32)
            fin = d.astype(bool)
            s[:, fin] = oracle.cartpole_reset(SEED, 0, tick, n)[:, fin]
            out = env.Read()
            assert np.array_equal(out.Observation.view(np.uint32), np.ascontiguousarray(s.T).view(np.uint32)), t
            assert np.array_equal(out.Reward, r) and np.array_equal(out.Done, fin), t
            model.push(s.T, d)
            ended += int(fin.sum()); explored += int(explore.sum())
        assert np.array_equal(actor.History(), model.h)
        assert ended > n and 0.25 * n * steps < explored < 0.35 * n * steps


def test_fused_actor_rollout_at_2_20_lanes(gpu_pkg):
    n, T = 1 << 20, 16
    rng = np.random.default_rng(11)
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True) as a, gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True) as b:
        a.Reset(); b.Reset()
        w, flat, pairs = _net(rng, RUNNER["CartPole-v1"])
        actor_a, actor_b = a.Actor(pairs, 4), b.Actor(pairs, 4)
        for t in range(T):
            actor_a.Step(0.1, 5, t)
        b.RolloutFusedDevice(None, T, actions="actor", epsilon=0.1, action_seed=5, action_tick0=0)
        assert np.array_equal(a.GetState().view(np.uint32), b.GetState().view(np.uint32))
        assert np.array_equal(actor_a.History(), actor_b.History())


def test_params_dataset_rows_map_to_the_actions_taken(gpu_pkg):
    n, S = 512, 4
    rng = np.random.default_rng(13)
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=60) as env:
        env.Reset()
        w, flat, pairs = _net(rng, RUNNER["CartPole-v1"])
        actor = env.Actor(pairs, S)
        mem = env.EpisodeMemory(capacity=32, max_length=60, history=S)
        for t in range(150):
            act = actor.Step(0.0, 1, t)
            mem.Push(act)
        x, action, _ = mem.BuildDataset("params", min_episodes=1)
        _, greedy = twin.forward(w, flat, _host(x))
        assert len(greedy) > 0 and np.array_equal(greedy, _host(action))


def test_refusals_write_nothing(gpu_pkg):
    import torch
    capi = gpu_pkg._capi if hasattr(gpu_pkg, "_capi") else __import__(gpu_pkg.__name__ + "._capi", fromlist=["x"])
    n = 1000
    rng = np.random.default_rng(17)
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True) as env:
        env.Reset()
        lib, h = env._lib, env._h
        out = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        # before any actor
        assert lib.gymnet_vecenv_actor_act_device(h, C.c_void_p(out.data_ptr()), None, 0.0, 0, 0) == capi.ERR_INVALID_ARG
        w, flat, pairs = _net(rng, [16, 50, 20, 2])
        widths = np.asarray(w, np.int32)
        def cfg(S, L, ws, f, count):
            return lib.gymnet_vecenv_actor_config(h, S, L, ws.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), count)
        assert cfg(4, 3, widths, flat, flat.size + 1) == capi.ERR_INVALID_ARG                   # count
        assert cfg(3, 3, widths, flat, flat.size) == capi.ERR_INVALID_ARG                       # widths[0] != S * obs_dim
        bad = widths.copy(); bad[1] = 65
        assert cfg(4, 3, bad, flat, flat.size) == capi.ERR_INVALID_ARG                          # width > 64
        assert cfg(4, 5, np.array([16, 8, 8, 8, 8, 2], np.int32), flat, flat.size) == capi.ERR_INVALID_ARG   # too many layers
        assert cfg(4, 3, widths, flat, flat.size) == capi.OK
        actor = env.Actor(pairs, 4)
        # push without a step
        hist0 = actor.History()
        assert lib.gymnet_vecenv_actor_push_device(h, None) == capi.ERR_INVALID_ARG
        assert np.array_equal(actor.History(), hist0)
        # a step without a push: act is refused and writes nothing; two steps: push is refused
        env.StepDevice(_dev(np.zeros(n, np.int32)))
        assert lib.gymnet_vecenv_actor_act_device(h, C.c_void_p(out.data_ptr()), None, 0.0, 0, 0) == capi.ERR_INVALID_ARG
        assert bool((out == -7).all())
        env.StepDevice(_dev(np.zeros(n, np.int32)))
        assert lib.gymnet_vecenv_actor_push_device(h, None) == capi.ERR_INVALID_ARG
        assert np.array_equal(actor.History(), hist0)
        spec = capi.RolloutSpec(struct_size=C.sizeof(capi.RolloutSpec), action_source=capi.ACTIONS_ACTOR, steps=4)
        assert lib.gymnet_vecenv_rollout_fused_ex_device(h, C.byref(spec)) == capi.ERR_INVALID_ARG     # stale history
        actor.Reset()
        # Load changes the actions, keeps the history
        a0 = _host(actor.Act()).copy()
        h1 = actor.History()
        w2, flat2, pairs2 = _net(np.random.default_rng(99), [16, 50, 20, 2])
        actor.Load(_dev(flat2))
        a1 = _host(actor.Act())
        assert np.array_equal(actor.History(), h1)
        _, g2 = twin.forward(w2, flat2, h1.reshape(n, -1))
        assert np.array_equal(a1, g2) and not np.array_equal(a0, a1)
    with gpu_pkg.VectorEnv("Pendulum-v1", 64, seed=SEED) as env:                                # a Box env
        f = np.zeros(3 * 1 + 1, np.float32)
        assert env._lib.gymnet_vecenv_actor_config(env._h, 1, 1, np.array([3, 1], np.int32).ctypes.data_as(C.c_void_p),
                                                   f.ctypes.data_as(C.c_void_p), f.size) == capi.ERR_UNSUPPORTED
    with gpu_pkg.VectorEnv("CartPole-v1", 256, seed=SEED, auto_reset=True, dtype=np.float64) as env:   # float64: no fused form
        env.Reset()
        env.Actor(_net(rng, [4, 2])[2], 1)
        spec = capi.RolloutSpec(struct_size=C.sizeof(capi.RolloutSpec), action_source=capi.ACTIONS_ACTOR, steps=4)
        assert env._lib.gymnet_vecenv_rollout_fused_ex_device(env._h, C.byref(spec)) == capi.ERR_UNSUPPORTED
