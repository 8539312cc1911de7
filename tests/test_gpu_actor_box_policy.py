"""GPU checks of the Box actor's policies (gym.net_amd/csrc/actor_box_policy.hip, gymnet_vecenv_actor_box_set_policy) on Pendulum and
MountainCarContinuous: act against the float64 twin (tests/_actor_box_policy_twin.py) under the four (head, explore) pairs, with handles
whose first global lane is 0, 5 and 2^32 + 6; sigma = 0; the default policy set explicitly against a handle that never set one; every one
of the 12 fused rollout forms (tests/_actor_box_policy_forms.py) under three policies against single closed-loop steps, bit for bit; one
fused rollout per env replayed on the CPU from its recorded actions; refusals and the policy's lifetime.  Every test fails without the
feature, at the missing export.

Batch 321: one full workgroup, a full wave and a one-lane partial wave.  History 2, net [2 * obs_dim, 16, 1] with the output layer scaled
so that about half of the outputs lie outside the bounds."""
import ctypes as C

import numpy as np
import pytest

import _actor_box_forms as box
import _actor_box_policy_forms as forms
import _actor_box_policy_twin as ptwin
import _actor_twin as twin
import _mountaincar_continuous_twin as mcc

pytestmark = pytest.mark.gpu
SEED = 0xAC7
F32 = np.float32
PENDULUM, MCC = "Pendulum-v1", "MountainCarContinuous-v0"
OBS_DIM = {PENDULUM: 3, MCC: 2}
N, S, SIGMA = 321, 2, 0.5
PAIRS = [("clamp", "sample"), ("clamp", "gaussian"), ("tanh", "sample"), ("tanh", "gaussian")]
bits = box.bits


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _net(name, x=None, seed=1):
    """(widths, flat, pairs) of a random [2 * obs_dim, 16, 1] network.  x: inputs [n, 2 * obs_dim] over which the output layer is scaled
    (row and bias, from the twin's numbers) so that the median |raw| is the bound; None: a fixed large scale."""
    widths = [S * OBS_DIM[name], 16, 1]
    w, flat, _ = twin.net(np.random.default_rng(seed), widths, scale=4.0)
    if x is not None:
        raw = twin.forward(w, flat, x)[0][:, 0].astype(np.float64)
        flat = flat.copy()
        flat[-17:] = (flat[-17:] * F32(box.BOUNDS[name][1] / np.median(np.abs(raw)))).astype(F32)
    return w, flat, twin.layers(widths, flat)


def _near_goal(env):
    """MountainCarContinuous: every third lane one step from the goal, so that episodes also end by termination"""
    if env.ObsDim != 2:
        return
    s = env.GetState()
    k = np.arange(env.NumberOfEnvironments) % 3 == 0
    s[0, k], s[1, k] = mcc.BELOW_GOAL32, F32(0.03)
    env.SetState(s)


@pytest.mark.parametrize("lane0", [0, 5, 2 ** 32 + 6])
@pytest.mark.parametrize("head,explore", PAIRS)
@pytest.mark.parametrize("name", [PENDULUM, MCC])
def test_act_equals_the_twin(gpu_pkg, name, head, explore, lane0):
    import torch
    low, high = box.BOUNDS[name]
    seed, tick = 77, 12
    with gpu_pkg.VectorEnv(name, N, seed=SEED, auto_reset=True, lane_offset=lane0) as env:
        x0 = twin.History(env.Reset(), S).x()
        w, flat, pairs = _net(name, x0)
        actor = env.Actor(pairs, history=S)
        actor.SetPolicy(head, explore, SIGMA)
        assert actor.Policy == (head, explore, SIGMA)
        want_raw = twin.forward(w, flat, actor.History().reshape(N, -1))[0]
        outside = (want_raw[:, 0] < low) | (want_raw[:, 0] > high)
        assert 0.2 < outside.mean() < 0.8                                    # the head works on both kinds of lane: from the twin's numbers
        wa, wb, wn = ptwin.words(seed, lane0, tick, N)
        raw = torch.empty((N, 1), dtype=torch.float32, device="cuda")
        greedy = None
        for eps in (0.0, 0.3, 1.0):
            raw.fill_(-7.0)
            torch.cuda.synchronize()                                         # the fill (torch's stream) ends before the handle's stream writes
            got = host(actor.Act(eps, seed=seed, tick=tick, logits=raw)).copy()
            assert got.dtype == np.float32 and got.shape == (N,)
            assert twin.same(host(raw), want_raw)                            # raw: the fmaf chain's bits, whatever the head
            want, bound, mask = ptwin.act64(want_raw[:, 0], wa, wb, wn, eps, low, high, head, explore, SIGMA)
            err = np.abs(got.astype(np.float64) - want)
            print(f"{name} {head} {explore} lane0 {lane0} eps {eps}: explore {int(mask.sum())}/{N}  max err {err.max():.3e}  "
                  f"max err/bound {np.max(err[bound > 0] / bound[bound > 0]) if (bound > 0).any() else 0.0:.3f}")
            assert np.all(err <= bound), (int(np.argmax(err - bound)), err.max())
            assert np.all((got >= low) & (got <= high))
            if eps == 0.0:
                greedy = got
                assert not mask.any()
                if head == "tanh":                                           # a smooth head: saturated outputs stay strictly inside
                    assert (np.abs(got) < high).mean() > 0.5
            else:
                differ = bits(got) != bits(greedy)
                assert not (differ & ~mask).any()                            # only lanes whose coin says so leave the greedy action
                assert differ[mask].mean() > 0.5                             # ... and they do
            if eps == 0.3:
                assert mask.any() and (~mask).any()
            if eps == 1.0:
                assert mask.all()


@pytest.mark.parametrize("head", ["clamp", "tanh"])
@pytest.mark.parametrize("name", [PENDULUM, MCC])
def test_sigma_zero_leaves_the_greedy_values(gpu_pkg, name, head):
    with gpu_pkg.VectorEnv(name, N, seed=SEED, auto_reset=True) as env:
        x0 = twin.History(env.Reset(), S).x()
        actor = env.Actor(_net(name, x0)[2], history=S)
        actor.SetPolicy(head, "gaussian", 0.0)
        greedy = host(actor.Act(0.0, seed=5, tick=3)).copy()
        noisy = host(actor.Act(1.0, seed=5, tick=3)).copy()
        assert np.array_equal(noisy, greedy)                                 # as values: clamp(greedy + 0 * z) == greedy
        actor.SetPolicy(head, "gaussian", SIGMA)
        assert (host(actor.Act(1.0, seed=5, tick=3)) != greedy).mean() > 0.5


def _fused(env, T, eps, seed, tick0):
    import torch
    n, O = env.NumberOfEnvironments, env.ObsDim
    rec = dict(rec_obs=torch.empty((T, O, n), dtype=torch.float32, device="cuda"), rec_reward=torch.empty((T, n), dtype=torch.float32, device="cuda"),
               rec_done=torch.empty((T, n), dtype=torch.uint8, device="cuda"), rec_actions=torch.empty((T, n), dtype=torch.float32, device="cuda"))
    env.RolloutFusedDevice(None, T, actions="actor", epsilon=eps, action_seed=seed, action_tick0=tick0, **rec)
    return {k: host(v) for k, v in rec.items()}


@pytest.mark.parametrize("name", [PENDULUM, MCC])
def test_the_default_policy_set_explicitly_changes_nothing(gpu_pkg, name):
    pairs = _net(name)[2]
    runs = []
    for setter in (None, lambda a: a.SetPolicy("clamp", "sample", 0.0),
                   lambda a: (a.SetPolicy("tanh", "gaussian", SIGMA), a.SetPolicy())):      # ... also after another policy
        with gpu_pkg.VectorEnv(name, N, seed=SEED, auto_reset=True) as env:
            env.Reset()
            actor = env.Actor(pairs, history=S)
            if setter:
                setter(actor)
            assert actor.Policy == ("clamp", "sample", 0.0)
            act = host(actor.Act(0.3, seed=5, tick=3)).copy()
            runs.append((env.KernelName(), act, _fused(env, 6, 0.3, 99, 1000), env.GetState(), actor.History()))
    for other in runs[1:]:
        assert other[0] == runs[0][0]
        assert np.array_equal(bits(other[1]), bits(runs[0][1]))
        for k, v in runs[0][2].items():
            assert np.array_equal(other[2][k].view(np.uint8), v.view(np.uint8)), k
        assert np.array_equal(bits(other[3]), bits(runs[0][3])) and np.array_equal(other[4], runs[0][4])


@pytest.mark.parametrize("policy", forms.POLICIES, ids=lambda p: "-".join(map(str, p)))
@pytest.mark.parametrize("row", forms.FORMS, ids=forms.form_id)
def test_every_form_equals_single_steps(gpu_pkg, row, policy):
    """T = 12 with max_episode_steps = 5 on the bookkeeping rows: lanes truncate and restart inside the launch (and MountainCarContinuous
    lanes put next to the goal terminate in its first step).  Both handles take 3 warm closed-loop steps under the default policy, so
    the rollout starts from a ring slot other than 0; then the comparison's after_warm callback — the one that receives the actor —
    moves the lanes, refills the history and sets the policy on each handle."""
    name = row["env"]
    kw = forms.handle_kwargs(row, limit=5)

    def with_policy(env, actor):
        _near_goal(env)
        actor.Reset()
        actor.SetPolicy(*policy)
    out = box.fused_equals_single_steps(gpu_pkg, name, N, 12, kw, row["shape"] == "records", _net(name)[2], S=S, eps=0.3, warm=3,
                                        after_warm=with_policy)
    low, high = box.BOUNDS[name]
    assert np.all((out["actions"] >= low) & (out["actions"] <= high))
    if row["shape"] != "lean":
        assert (out["done"] & 2).any()
        if row["auto_reset"]:
            assert (out["done"] & 2).sum(axis=0).max() >= 2                   # a lane truncates, restarts and truncates again
    if name == MCC:
        assert (out["done"][0][np.arange(N) % 3 == 0] & 1).all()


def test_pendulum_rollout_equals_the_teacher_forced_replay(gpu_pkg, oracle):
    T = 12
    with gpu_pkg.VectorEnv(PENDULUM, N, seed=SEED) as env:
        env.Reset()
        actor = env.Actor(_net(PENDULUM)[2], history=S)
        actor.SetPolicy("tanh", "gaussian", SIGMA)
        state = env.GetState()
        got = _fused(env, T, 0.3, 99, 1000)
        for t in range(T):
            state, obs, rw, dn = oracle.env_step(PENDULUM, state, got["rec_actions"][t], dtype=np.float32)
            assert np.array_equal(bits(got["rec_obs"][t]), bits(obs)), t
            assert np.array_equal(bits(got["rec_reward"][t]), bits(rw)) and np.array_equal(got["rec_done"][t], dn), t
        assert np.array_equal(bits(env.GetState()), bits(state))
        assert len(np.unique(got["rec_actions"])) > T * N // 2                # actions of a continuous policy, not a few clamped values


def test_mountaincar_continuous_rollout_equals_the_teacher_forced_replay(gpu_pkg):
    T = 12
    with gpu_pkg.VectorEnv(MCC, N, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=5) as env:
        env.Reset()
        _near_goal(env)
        actor = env.Actor(_net(MCC)[2], history=S)
        actor.SetPolicy("tanh", "gaussian", SIGMA)
        tick0 = env.Tick
        rp = mcc.Replay(env.GetState(), SEED, 0, True, True, 5)
        got = _fused(env, T, 0.3, 99, 1000)
        for t in range(T):
            obs, rw, db, fin = rp.step(got["rec_actions"][t], tick0 + t)
            assert np.array_equal(bits(got["rec_obs"][t]), bits(obs)), t
            assert np.array_equal(bits(got["rec_reward"][t]), bits(rw)) and np.array_equal(got["rec_done"][t], db), t
        assert (got["rec_done"] & 1).any() and (got["rec_done"] & 2).any()


def test_refusals_and_the_policys_lifetime(gpu_pkg):
    import importlib
    import torch
    capi = importlib.import_module(gpu_pkg.__name__ + "._capi")
    TANH, GAUSS = capi.BOX_HEAD_TANH, capi.BOX_EXPLORE_GAUSSIAN

    def get(lib, h):
        head, explore, sigma = C.c_int32(-9), C.c_int32(-9), C.c_float(-9.0)
        return lib.gymnet_vecenv_actor_box_get_policy(h, C.byref(head), C.byref(explore), C.byref(sigma)), (head.value, explore.value, sigma.value)

    with gpu_pkg.VectorEnv("CartPole-v1", N, seed=SEED, auto_reset=True) as env:          # a Discrete actor
        env.Reset()
        lib, h = env._lib, env._h
        assert lib.gymnet_vecenv_actor_box_set_policy(h, TANH, GAUSS, 0.5) == capi.ERR_INVALID_ARG       # no actor
        assert get(lib, h) == (capi.ERR_INVALID_ARG, (-9, -9, -9.0))
        actor = env.Actor(twin.net(np.random.default_rng(2), [4, 2])[2], 1)
        before = host(actor.Act(0.3, 5, 3)).copy()
        assert lib.gymnet_vecenv_actor_box_set_policy(h, TANH, GAUSS, 0.5) == capi.ERR_INVALID_ARG
        assert b"Discrete" in lib.gymnet_last_error()
        assert get(lib, h) == (capi.ERR_INVALID_ARG, (-9, -9, -9.0))
        assert np.array_equal(host(actor.Act(0.3, 5, 3)), before)
        with pytest.raises(ValueError):
            actor.SetPolicy("tanh", "gaussian", 0.5)
    with gpu_pkg.VectorEnv(PENDULUM, N, seed=SEED) as env:
        env.Reset()
        lib, h = env._lib, env._h
        assert lib.gymnet_vecenv_actor_box_set_policy(h, TANH, GAUSS, 0.5) == capi.ERR_INVALID_ARG       # no actor
        assert b"gymnet_vecenv_actor_box_config" in lib.gymnet_last_error()
        assert get(lib, h) == (capi.ERR_INVALID_ARG, (-9, -9, -9.0))
        w, flat, pairs = _net(PENDULUM)
        actor = env.Actor(pairs, history=S)
        assert get(lib, h) == (capi.OK, (0, 0, 0.0)) and actor.Policy == ("clamp", "sample", 0.0)
        actor.SetPolicy("tanh", "gaussian", 0.25)
        assert get(lib, h) == (capi.OK, (TANH, GAUSS, 0.25))
        assert lib.gymnet_vecenv_actor_box_get_policy(h, None, None, None) == capi.OK                    # any out pointer may be null
        before = host(actor.Act(0.3, 5, 3)).copy()
        hist, state, tick = actor.History(), env.GetState(), env.Tick
        for head, explore, sigma in ((2, GAUSS, 0.5), (-1, GAUSS, 0.5), (TANH, 2, 0.5), (TANH, -1, 0.5), (TANH, GAUSS, float("nan")),
                                     (TANH, GAUSS, -1.0), (TANH, GAUSS, float("inf")), (0, 0, float("-inf"))):
            assert lib.gymnet_vecenv_actor_box_set_policy(h, head, explore, sigma) == capi.ERR_INVALID_ARG, (head, explore, sigma)
            assert get(lib, h) == (capi.OK, (TANH, GAUSS, 0.25))
        assert np.array_equal(bits(host(actor.Act(0.3, 5, 3))), bits(before))
        assert np.array_equal(actor.History(), hist) and np.array_equal(bits(env.GetState()), bits(state)) and env.Tick == tick
        # sigma is stored whatever explore is
        actor.SetPolicy("clamp", "sample", 0.75)
        assert actor.Policy == ("clamp", "sample", 0.75)
        actor.SetPolicy("tanh", "gaussian", 0.25)
        # no staleness state changes: a stale history stays stale through set_policy, and a push is still what cures it
        poison = torch.full((N,), -7.0, dtype=torch.float32, device="cuda")
        env.StepDevice(actor.Act(0.3, 5, 3))
        actor.SetPolicy("tanh", "gaussian", 0.5)
        assert lib.gymnet_vecenv_actor_box_act_device(h, C.c_void_p(poison.data_ptr()), None, 0.0, 0, 0) == capi.ERR_INVALID_ARG
        assert bool((poison == -7.0).all())
        actor.Push()                                                                                     # push, reset and load keep the policy
        assert actor.Policy == ("tanh", "gaussian", 0.5)
        actor.Reset()
        actor.Load(pairs)
        actor.Load(torch.from_numpy(flat).cuda())
        assert actor.Policy == ("tanh", "gaussian", 0.5)
        noisy = host(actor.Act(1.0, 5, 4)).copy()
        assert (noisy != host(actor.Act(0.0, 5, 4))).mean() > 0.5
        again = env.Actor(pairs, history=S)                                                              # a re-config returns to the default
        assert again.Policy == ("clamp", "sample", 0.0) and get(lib, h) == (capi.OK, (0, 0, 0.0))
