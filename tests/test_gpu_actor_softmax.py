"""GPU checks of a Discrete actor's softmax exploration (gym.net_amd/csrc/actor_softmax.hip, gymnet_vecenv_actor_set_exploration) on
CartPole, MountainCar and Acrobot.  The draw is specified in float32, so every comparison with the C twin
(tests/_actor_softmax_twin.py) is bit for bit: act against the twin for epsilon in {0, 0.3, 1} x temperature in {0.25, 1, 4} with handles
whose first global lane is 0, 5 and 2^32 + 6; epsilon = 0 under softmax against the default; the default set explicitly against a handle
that never set anything; every one of the 18 fused rollout forms (tests/_actor_softmax_forms.py) under the default and two softmax
settings against single closed-loop steps; one fused rollout per env replayed teacher-forced through the twin from its recorded
observations and actions; actor.Step(repeat=2) and EpisodeMemory.Rollout(actions="actor") under softmax against their unfused loops;
refusals and the setting's lifetime.  Every test fails without the feature, at the missing export.

Batch 321 (257 with the attachments): full waves and a one-lane partial wave.  History 2, net [2 * obs_dim, 16, A] with the output layer
scaled — from the twin's numbers, over the handle's own inputs or over inputs like those after a reset — so that the median spread of the
logits is 0.5: at temperature 0.25 the least likely action of a typical lane still has a few percent, so every action occurs, and at
temperature 4 the draw is close to uniform."""
import ctypes as C

import numpy as np
import pytest

import _actor_softmax_forms as forms
import _actor_softmax_twin as stwin
import _actor_twin as twin

pytestmark = pytest.mark.gpu
SEED = 0xAC7
F32 = np.float32
CARTPOLE, MOUNTAINCAR, ACROBOT = "CartPole-v1", "MountainCar-v0", "Acrobot-v1"
DIMS = forms.DIMS
N, S = 321, 2
host = forms.forms.host


def _typical(name, n=512):
    """inputs [n, 2 * obs_dim] like those after a reset (both history slots hold the first observation), drawn on the host"""
    rng = np.random.default_rng(0)
    if name == CARTPOLE:
        obs = rng.uniform(-0.05, 0.05, (n, 4))
    elif name == MOUNTAINCAR:
        obs = np.stack([rng.uniform(-0.6, -0.4, n), np.zeros(n)], axis=1)
    else:
        s = rng.uniform(-0.1, 0.1, (n, 4))
        obs = np.stack([np.cos(s[:, 0]), np.sin(s[:, 0]), np.cos(s[:, 1]), np.sin(s[:, 1]), s[:, 2], s[:, 3]], axis=1)
    return np.tile(obs.astype(F32), (1, S))


def _net(name, x=None, seed=1):
    """(widths, flat, pairs) of a random [2 * obs_dim, 16, A] network whose output layer (rows and biases) is scaled so that the median of
    max - min of the logits over the inputs x [n, 2 * obs_dim] is 0.5; None: over _typical(name)."""
    O, A = DIMS[name]
    widths = [S * O, 16, A]
    w, flat, _ = twin.net(np.random.default_rng(seed), widths, scale=2.0)
    logits = twin.forward(w, flat, _typical(name) if x is None else x)[0].astype(np.float64)
    flat = flat.copy()
    flat[-17 * A:] = (flat[-17 * A:] * F32(0.5 / np.median(logits.max(axis=1) - logits.min(axis=1)))).astype(F32)
    return w, flat, twin.layers(widths, flat)


@pytest.mark.parametrize("lane0", [0, 5, 2 ** 32 + 6])
@pytest.mark.parametrize("name", [CARTPOLE, MOUNTAINCAR, ACROBOT])
def test_act_equals_the_twin(gpu_pkg, name, lane0):
    import torch
    A = DIMS[name][1]
    seed, tick = 77, 12
    with gpu_pkg.VectorEnv(name, N, seed=SEED, auto_reset=True, lane_offset=lane0) as env:
        x0 = twin.History(env.Reset(), S).x()
        w, flat, pairs = _net(name, x0)
        actor = env.Actor(pairs, history=S)
        want_logits, want_greedy = twin.forward(w, flat, actor.History().reshape(N, -1))
        wa, wb = stwin.words(seed, lane0, tick, N)
        logits = torch.empty((N, A), dtype=torch.float32, device="cuda")
        for tau in (0.25, 1.0, 4.0):
            actor.SetExploration("softmax", tau)
            assert actor.Exploration == ("softmax", tau)
            for eps in (0.0, 0.3, 1.0):
                logits.fill_(-7.0)
                torch.cuda.synchronize()                                     # the fill (torch's stream) ends before the handle's stream writes
                got = host(actor.Act(eps, seed=seed, tick=tick, logits=logits)).copy()
                assert got.dtype == np.int32 and got.shape == (N,)
                assert twin.same(host(logits), want_logits)                  # the logits: the fmaf chain's bits
                want, mask, greedy = stwin.act(want_logits, wa, wb, eps, "softmax", tau)
                assert np.array_equal(greedy, want_greedy)
                print(f"{name} lane0 {lane0} tau {tau} eps {eps}: explore {int(mask.sum())}/{N}  off greedy {int((want != greedy).sum())}  "
                      f"counts {np.bincount(want, minlength=A).tolist()}  mismatches {int((got != want).sum())}")
                assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]     # bit-equal to the twin, no lane exempted
                if eps == 0.0:
                    assert not mask.any() and np.array_equal(want, greedy)
                if eps == 0.3:
                    assert mask.any() and (~mask).any() and np.array_equal(want[~mask], greedy[~mask])
                if eps == 1.0:                                               # from the twin's side: not a saturated net
                    assert mask.all() and len(np.unique(want)) == A and (want != greedy).any()
                    assert not np.array_equal(want, stwin.uniform(wa, A))    # ... and not the uniform draw either


@pytest.mark.parametrize("name", [CARTPOLE, MOUNTAINCAR, ACROBOT])
def test_epsilon_zero_and_the_default_set_explicitly_change_nothing(gpu_pkg, name):
    import torch
    pairs = _net(name)[2]
    T = 6

    def fused(env):
        rec = dict(rec_obs=torch.empty((T, env.ObsDim, N), dtype=torch.float32, device="cuda"), rec_done=torch.empty((T, N), dtype=torch.uint8, device="cuda"),
                   rec_actions=torch.empty((T, N), dtype=torch.int32, device="cuda"))
        env.RolloutFusedDevice(None, T, actions="actor", epsilon=0.3, action_seed=99, action_tick0=1000, **rec)
        return {k: host(v) for k, v in rec.items()}
    runs = []
    for setter in (None, lambda a: a.SetExploration("uniform", 1.0),
                   lambda a: (a.SetExploration("softmax", 0.5), a.SetExploration()),      # ... also after softmax
                   lambda a: a.SetExploration("uniform", 0.25)):                          # the temperature does not matter to "uniform"
        with gpu_pkg.VectorEnv(name, N, seed=SEED, auto_reset=True) as env:
            env.Reset()
            actor = env.Actor(pairs, history=S)
            if setter:
                setter(actor)
            assert actor.Exploration[0] == "uniform"
            act = host(actor.Act(0.3, seed=5, tick=3)).copy()
            runs.append((env.KernelName(), act, fused(env), env.GetState(), actor.History()))
            greedy = host(actor.Act(0.0, seed=5, tick=3)).copy()
            actor.SetExploration("softmax", 0.5)                              # epsilon = 0 under softmax: the argmax, as by default
            assert np.array_equal(host(actor.Act(0.0, seed=5, tick=3)), greedy)
            assert not np.array_equal(host(actor.Act(1.0, seed=5, tick=3)), greedy)
    for other in runs[1:]:
        assert other[0] == runs[0][0]
        assert np.array_equal(other[1], runs[0][1])
        for k, v in runs[0][2].items():
            assert np.array_equal(other[2][k].view(np.uint8), v.view(np.uint8)), k
        assert np.array_equal(other[3].view(np.uint32), runs[0][3].view(np.uint32)) and np.array_equal(other[4], runs[0][4])


def _at_the_goal(env):
    """MountainCar / Acrobot lanes do not end on their own within a dozen steps: every third lane starts where its next step is terminal"""
    s = env.GetState()
    third = np.arange(s.shape[1]) % 3 == 0
    if env.ObsDim == 2:
        s[0, third], s[1, third] = 0.49, 0.05
    elif env.ObsDim == 6:
        s[:, third] = np.array([np.pi, 0.0, 0.0, 0.0], F32)[:, None]
    else:
        return
    env.SetState(s)


@pytest.mark.parametrize("setting", forms.SETTINGS, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("row", forms.FORMS, ids=forms.form_id)
def test_every_form_equals_single_steps(gpu_pkg, row, setting):
    """T = 12 with max_episode_steps = 5 on the bookkeeping rows: lanes truncate and restart inside the launch (and MountainCar / Acrobot
    lanes put at the goal terminate in its first step).  Both handles take 3 warm closed-loop steps under the default setting, so the
    rollout starts from a ring slot other than 0; then the lanes are moved, the history refilled and the setting set on each handle —
    the default row goes through softmax and back."""
    name = row["env"]
    kw = forms.handle_kwargs(row, limit=5)

    def with_setting(env, actor):
        _at_the_goal(env)
        actor.Reset()
        if setting[0] == "uniform":
            actor.SetExploration("softmax", 0.5)
        actor.SetExploration(*setting)
    out = forms.fused_equals_single_steps(gpu_pkg, name, N, 12, kw, row["shape"] == "records", _net(name)[2], S=S, eps=0.5, warm=3,
                                          after_warm=with_setting)
    A = DIMS[name][1]
    assert ((out["actions"] >= 0) & (out["actions"] < A)).all() and len(np.unique(out["actions"])) == A
    if row["shape"] != "lean":
        assert (out["done"] & 2).any()
        if row["auto_reset"]:
            assert (out["done"] & 2).sum(axis=0).max() >= 2                   # a lane truncates, restarts and truncates again
    if name != CARTPOLE:
        assert (out["done"][0][np.arange(N) % 3 == 0] & 1).all()


@pytest.mark.parametrize("name", [CARTPOLE, MOUNTAINCAR, ACROBOT])
def test_a_fused_rollout_replays_teacher_forced_through_the_twin(gpu_pkg, name):
    """From the recorded observations and done bytes the history of every step is rebuilt on the host, the fmaf twin gives its logits, the
    softmax twin its action with the words of (action_seed, lane, action_tick0 + t): the recorded actions, bit for bit."""
    import torch
    T, eps, tau, aseed, tick0, lane0 = 12, 0.6, 0.5, 99, 1000, 7
    A = DIMS[name][1]
    w, flat, pairs = _net(name)
    with gpu_pkg.VectorEnv(name, N, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=5, lane_offset=lane0) as env:
        obs0 = env.Reset()
        actor = env.Actor(pairs, history=S)
        actor.SetExploration("softmax", tau)
        rec = dict(rec_obs=torch.empty((T, env.ObsDim, N), dtype=torch.float32, device="cuda"), rec_done=torch.empty((T, N), dtype=torch.uint8, device="cuda"),
                   rec_actions=torch.empty((T, N), dtype=torch.int32, device="cuda"))
        env.RolloutFusedDevice(None, T, actions="actor", epsilon=eps, action_seed=aseed, action_tick0=tick0, **rec)
        got = {k: host(v) for k, v in rec.items()}
        model = twin.History(obs0, S)
        off_greedy = 0
        for t in range(T):
            logits, greedy = twin.forward(w, flat, model.x())
            wa, wb = stwin.words(aseed, lane0, tick0 + t, N)
            want, mask, _ = stwin.act(logits, wa, wb, eps, "softmax", tau)
            assert np.array_equal(got["rec_actions"][t], want), t
            off_greedy += int((want != greedy).sum())
            model.push(got["rec_obs"][t].T, got["rec_done"][t])
        assert np.array_equal(actor.History(), model.h)
        assert off_greedy > 0 and len(np.unique(got["rec_actions"])) == A and (got["rec_done"] & 2).any()


ATT = dict(seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=9)


def test_actor_step_with_repeat_under_softmax_equals_the_unfused_loop(gpu_pkg):
    n = 257
    pairs = _net(CARTPOLE, seed=4)[2]
    with gpu_pkg.VectorEnv(CARTPOLE, n, **ATT) as f, gpu_pkg.VectorEnv(CARTPOLE, n, **ATT) as e:
        f.Reset(); e.Reset()
        fa, ea = f.Actor(pairs, history=S), e.Actor(pairs, history=S)
        fa.SetExploration("softmax", 0.5); ea.SetExploration("softmax", 0.5)
        moved = 0
        for d in range(12):
            got = host(fa.Step(0.5, 77, d, repeat=2)).copy()
            greedy = host(ea.Act(0.0, 77, d)).copy()
            want = ea.Act(0.5, 77, d)
            e.StepRepeatDevice(want, 2)
            ea.Push()
            assert np.array_equal(got, host(want)), d
            moved += int((got != greedy).sum())
            assert np.array_equal(f.GetState(), e.GetState()) and f.Tick == e.Tick == 1 + 3 * (d + 1)
            assert np.array_equal(fa.History(), ea.History()), d
        assert moved > 0 and (f.GetArray("finished_length") > 0).any()


def test_memory_rollout_under_softmax_equals_single_steps_and_pushes(gpu_pkg):
    n, T = 257, 24
    pairs = _net(CARTPOLE, seed=5)[2]
    snaps = []
    for fused in (False, True):
        with gpu_pkg.VectorEnv(CARTPOLE, n, **ATT) as env:
            env.Reset()
            actor = env.Actor(pairs, history=S)
            actor.SetExploration("softmax", 0.5)
            mem = env.EpisodeMemory(capacity=5, max_length=9, history=S, rollout_chunk=16)
            if fused:
                taken = host(mem.Rollout(T, actions="actor", action_seed=77, action_tick0=1000, epsilon=0.5)).copy()
            else:
                taken = np.stack([host(a).copy() for a in (_step_and_push(actor, mem, 0.5, 77, 1000 + t) for t in range(T))])
            x, a, onehot, r = (host(v) for v in mem.BuildDataset("params", min_episodes=0, reward=True))
            snaps.append(dict(taken=taken, stats=mem.Stats(), episodes=mem.Episodes(), x=x, a=a, onehot=onehot, r=r, state=env.GetState(),
                              hist=actor.History(), tick=env.Tick))
    a, b = snaps
    assert a["stats"] == b["stats"] and a["stats"]["ended"] > 5 and a["stats"]["kept"] == 5
    assert np.array_equal(a["taken"], b["taken"]) and len(np.unique(a["taken"])) == 2
    for g, w_ in zip(a["episodes"], b["episodes"]):
        assert np.array_equal(g, w_)
    assert len(a["x"]) > 0
    for k in ("x", "a", "onehot", "r", "state", "hist"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    assert a["tick"] == b["tick"]


def _step_and_push(actor, mem, eps, seed, tick):
    acts = actor.Step(eps, seed, tick)
    mem.Push(acts)
    return acts


def test_refusals_and_the_settings_lifetime(gpu_pkg):
    import importlib
    import torch
    capi = importlib.import_module(gpu_pkg.__name__ + "._capi")
    SOFTMAX, UNIFORM = capi.ACTOR_EXPLORE_SOFTMAX, capi.ACTOR_EXPLORE_UNIFORM

    def get(lib, h):
        explore, temperature = C.c_int32(-9), C.c_float(-9.0)
        return lib.gymnet_vecenv_actor_get_exploration(h, C.byref(explore), C.byref(temperature)), (explore.value, temperature.value)

    with gpu_pkg.VectorEnv("Pendulum-v1", N, seed=SEED) as env:                           # a Box actor
        env.Reset()
        lib, h = env._lib, env._h
        assert lib.gymnet_vecenv_actor_set_exploration(h, SOFTMAX, 1.0) == capi.ERR_INVALID_ARG           # no actor
        assert get(lib, h) == (capi.ERR_INVALID_ARG, (-9, -9.0))
        actor = env.Actor(twin.net(np.random.default_rng(2), [3, 1])[2], 1)
        before = host(actor.Act(0.3, 5, 3)).copy()
        assert lib.gymnet_vecenv_actor_set_exploration(h, SOFTMAX, 1.0) == capi.ERR_INVALID_ARG
        assert b"Box" in lib.gymnet_last_error()
        assert get(lib, h) == (capi.ERR_INVALID_ARG, (-9, -9.0))
        assert np.array_equal(host(actor.Act(0.3, 5, 3)).view(np.uint32), before.view(np.uint32))
        assert actor.Policy == ("clamp", "sample", 0.0)
        with pytest.raises(ValueError):
            actor.SetExploration("softmax", 1.0)
    with gpu_pkg.VectorEnv(CARTPOLE, N, seed=SEED) as env:
        env.Reset()
        lib, h = env._lib, env._h
        assert lib.gymnet_vecenv_actor_set_exploration(h, SOFTMAX, 1.0) == capi.ERR_INVALID_ARG           # no actor
        assert b"gymnet_vecenv_actor_config" in lib.gymnet_last_error()
        assert get(lib, h) == (capi.ERR_INVALID_ARG, (-9, -9.0))
        w, flat, pairs = _net(CARTPOLE)
        actor = env.Actor(pairs, history=S)
        assert get(lib, h) == (capi.OK, (UNIFORM, 1.0)) and actor.Exploration == ("uniform", 1.0)
        actor.SetExploration("softmax", 0.25)
        assert get(lib, h) == (capi.OK, (SOFTMAX, 0.25))
        assert lib.gymnet_vecenv_actor_get_exploration(h, None, None) == capi.OK                          # any out pointer may be null
        before = host(actor.Act(0.5, 5, 3)).copy()
        hist, state, tick = actor.History(), env.GetState(), env.Tick
        for explore, temperature in ((2, 1.0), (-1, 1.0), (SOFTMAX, float("nan")), (SOFTMAX, 0.0), (SOFTMAX, -0.0), (SOFTMAX, -1.0),
                                     (SOFTMAX, float("inf")), (UNIFORM, float("-inf")), (SOFTMAX, 1e-39), (UNIFORM, 0.0)):
            assert lib.gymnet_vecenv_actor_set_exploration(h, explore, C.c_float(temperature)) == capi.ERR_INVALID_ARG, (explore, temperature)
            assert get(lib, h) == (capi.OK, (SOFTMAX, 0.25))
        assert np.array_equal(host(actor.Act(0.5, 5, 3)), before)                                         # a refusal changes no action
        assert np.array_equal(actor.History(), hist) and np.array_equal(env.GetState().view(np.uint32), state.view(np.uint32)) and env.Tick == tick
        with pytest.raises(ValueError):                                                                   # a Discrete actor has no Box policy
            actor.SetPolicy("tanh", "gaussian", 0.3)
        assert lib.gymnet_vecenv_actor_box_set_policy(h, 1, 1, C.c_float(0.3)) == capi.ERR_INVALID_ARG
        # the temperature is stored whatever explore is
        actor.SetExploration("uniform", 0.75)
        assert actor.Exploration == ("uniform", 0.75)
        actor.SetExploration("softmax", 0.25)
        # no staleness state changes: a stale history stays stale through set_exploration, and a push is still what cures it
        poison = torch.full((N,), -7, dtype=torch.int32, device="cuda")
        env.StepDevice(actor.Act(0.5, 5, 3))
        actor.SetExploration("softmax", 0.5)
        assert lib.gymnet_vecenv_actor_act_device(h, C.c_void_p(poison.data_ptr()), None, C.c_float(0.0), 0, 0) == capi.ERR_INVALID_ARG
        assert bool((poison == -7).all())
        actor.Push()                                                                                     # push, reset and load keep the setting
        assert actor.Exploration == ("softmax", 0.5)
        actor.Reset()
        actor.Load(pairs)
        actor.Load(torch.from_numpy(flat).cuda())
        assert actor.Exploration == ("softmax", 0.5)
        sampled = host(actor.Act(1.0, 5, 4)).copy()
        logits = twin.forward(w, flat, actor.History().reshape(N, -1))[0]
        wa, wb = stwin.words(5, 0, 4, N)
        assert np.array_equal(sampled, stwin.act(logits, wa, wb, 1.0, "softmax", 0.5)[0])
        again = env.Actor(pairs, history=S)                                                              # a re-config returns to the default
        assert again.Exploration == ("uniform", 1.0) and get(lib, h) == (capi.OK, (UNIFORM, 1.0))
        assert np.array_equal(host(again.Act(1.0, 5, 4)), stwin.uniform(wa, 2))
