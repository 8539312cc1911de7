"""GPU checks of the actor (gym.net_amd/csrc/actor.hip, gymnet_vecenv_actor_*): logits and greedy actions bit-identical to the fmaf twin
(tests/_actor_twin.py, -0 == +0) on CartPole / MountainCar / Acrobot float32 and CartPole float64 handles; epsilon-greedy actions equal
to ComposeActionsDevice over the twin's greedy actions; the history against the NumPy model of its rules; the fused rollout with
GYMNET_ACTIONS_ACTOR bit-identical to steps x (Act, StepDevice, Push) on plain, trainer-shaped and done-list / terminal-observation
handles, episode records with their returns and lengths included; a closed loop against the oracle's step and Philox streams; params datasets of an
EpisodeMemory whose rows the twin maps to the actions taken; refusals that write nothing; Load."""
import ctypes as C

import numpy as np
import pytest

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


def _net(rng, widths):
    w, flat = twin.random_net(rng, widths, scale=2.0)
    pairs, p = [], 0
    for l in range(len(widths) - 1):
        win, wout = widths[l], widths[l + 1]
        pairs.append((flat[p:p + win * wout].reshape(wout, win), flat[p + win * wout:p + win * wout + wout]))
        p += win * wout + wout
    return w, flat, pairs


def _warm(env, actor, steps, rng):
    """a few random steps with pushes, so the histories differ from slot to slot"""
    n = env.NumberOfEnvironments
    for t in range(steps):
        env.StepDevice(_dev(rng.integers(0, env.ActionSpace.N, n).astype(np.int32)))
        actor.Push()


def _same(a, b):
    """bit equality with -0 == +0"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.array_equal(a == 0, b == 0) and np.array_equal(np.where(a == 0, 0, a).view(np.uint32), np.where(b == 0, 0, b).view(np.uint32))


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


@pytest.mark.parametrize("auto_reset", [True, False])
def test_history_follows_the_rules(gpu_pkg, auto_reset):
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
            actor.Push()
            model.push(out.Observation, d)
            if not auto_reset and d.any():
                obs = env.ResetWhere(d)
                actor.Reset(_dev(d))
                model.reset(obs, d)
            assert np.array_equal(actor.History(), model.h), t


def _trainer(gpu_pkg, name, n, trainer):
    """plain auto-reset; the trainer's shape (EPISODE_STATS, max_episode_steps); "full": that plus the done list and terminal observations"""
    kw = dict(auto_reset=True)
    if trainer:
        kw.update(episode_stats=True, max_episode_steps=50)
    if trainer == "full":
        kw.update(done_list=True, final_obs=True)
    return gpu_pkg.VectorEnv(name, n, seed=SEED, **kw)


@pytest.mark.parametrize("name", ["CartPole-v1", "MountainCar-v0", "Acrobot-v1"])
@pytest.mark.parametrize("T", [1, 7, 64])
@pytest.mark.parametrize("trainer", [False, True, "full"])
def test_fused_actor_rollout_equals_single_steps(gpu_pkg, name, T, trainer, n=3000):
    import torch
    rng = np.random.default_rng(T)
    with _trainer(gpu_pkg, name, n, trainer) as a, _trainer(gpu_pkg, name, n, trainer) as b:
        a.Reset(); b.Reset()
        O, A = a.ObsDim, a.ActionSpace.N
        w, flat, pairs = _net(rng, [4 * O] + RUNNER[name][1:-1] + [A])
        actor_a, actor_b = a.Actor(pairs, 4), b.Actor(pairs, 4)
        eps, seed, tick0 = 0.3, 99, 1000
        obs_a, rew_a, done_a, act_a, fin_a = [], [], [], [], []
        for t in range(T):
            act_a.append(_host(actor_a.Step(eps, seed, tick0 + t)).copy())
            r = a.Read()
            obs_a.append(r.Observation.T.copy()); rew_a.append(r.Reward.copy()); done_a.append(a.GetArray("done").copy())
            if trainer:                                                   # the finished episodes' (return, length) of this step
                fin_a.append((a.GetArray("finished_return").copy(), a.GetArray("finished_length").copy()))
        rec_obs = torch.empty((T, O, n), dtype=torch.float32, device="cuda")
        rec_rew = torch.empty((T, n), dtype=torch.float32, device="cuda")
        rec_done = torch.empty((T, n), dtype=torch.uint8, device="cuda")
        rec_act = torch.empty((T, n), dtype=torch.int32, device="cuda")
        ep = None
        if trainer:
            cap = T * n                                                     # at most one episode per lane and step
            ep = dict(step=torch.empty(cap, dtype=torch.int32, device="cuda"), lane=torch.empty(cap, dtype=torch.int32, device="cuda"),
                      ret=torch.empty(cap, dtype=torch.float32, device="cuda"), length=torch.empty(cap, dtype=torch.int32, device="cuda"),
                      capacity=cap, count=torch.zeros(2, dtype=torch.int32, device="cuda"))
        b.RolloutFusedDevice(None, T, actions="actor", epsilon=eps, action_seed=seed, action_tick0=tick0, rec_obs=rec_obs, rec_reward=rec_rew,
                             rec_done=rec_done, rec_actions=rec_act, episodes=ep)
        assert np.array_equal(_host(rec_act), np.stack(act_a))
        assert np.array_equal(_host(rec_obs).view(np.uint32), np.stack(obs_a).astype(np.float32).view(np.uint32))
        assert np.array_equal(_host(rec_rew).view(np.uint32), np.stack(rew_a).view(np.uint32))
        assert np.array_equal(_host(rec_done), np.stack(done_a))
        assert np.array_equal(a.GetState().view(np.uint32), b.GetState().view(np.uint32))
        assert np.array_equal(a.GetArray("done"), b.GetArray("done"))
        assert a.Tick == b.Tick
        assert np.array_equal(actor_a.History(), actor_b.History())
        if trainer:
            for k in ("episode_return", "episode_length", "finished_return", "finished_length"):
                assert np.array_equal(a.GetArray(k), b.GetArray(k)), k
            cnt = _host(ep["count"]).astype(np.int64)
            m = int(cnt[0])
            got = sorted(zip(_host(ep["step"])[:m].tolist(), _host(ep["lane"])[:m].tolist(), _host(ep["ret"])[:m].tolist(), _host(ep["length"])[:m].tolist()))
            want = []
            for t in range(T):
                for lane in np.nonzero(done_a[t])[0]:
                    want.append((t, int(lane), float(fin_a[t][0][lane]), int(fin_a[t][1][lane])))
            assert int(cnt[1]) == len(want) and got == sorted(want)              # step, lane, return and length of every record
        if trainer == "full":                                                     # the last step's done list and terminal observations
            assert np.array_equal(a.GetArray("final_obs").view(np.uint32), b.GetArray("final_obs").view(np.uint32))
            assert np.array_equal(np.sort(a.DoneLanes()), np.sort(b.DoneLanes()))
            ra, rb = a.DoneRecords(), b.DoneRecords()
            ka, kb = np.argsort(ra["lanes"]), np.argsort(rb["lanes"])
            for k in ("lanes", "return", "length", "final_obs"):
                assert np.array_equal(ra[k][ka], rb[k][kb]), k
        # the history is current after the fused rollout: the next single step is accepted on both
        assert np.array_equal(_host(actor_a.Step(eps, seed, tick0 + T)), _host(actor_b.Step(eps, seed, tick0 + T)))


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
