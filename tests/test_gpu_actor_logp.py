"""GPU checks of the log-probability a Discrete actor records (gym.net_amd/csrc/actor_logp.hip, gymnet_vecenv_actor_act_logp_device and
gymnet_vecenv_rollout_fused_logp_device) on CartPole, MountainCar and Acrobot.  The quantity is specified in float32, so every comparison
with the C twin (tests/_actor_logp_twin.py) is on uint32 views: act with logp against the twin for handles whose first global lane is 0, 5
and 2^32 + 6, under five settings and three epsilons, with actions and logits equal to Act without logp, and on a float64 CartPole handle;
every one of the 18 fused rollout forms (tests/_actor_logp_forms.py) under the default and two softmax settings against single closed-loop
steps with logp; one fused rollout per env replayed teacher-forced through the twins; non-finite logits; the NULL forwarders; refusals
that write nothing; actor.Step(repeat=2, logp=) and EpisodeMemory.Rollout(actions="actor", rec_logp=) against their unfused loops.  Every
test fails without the feature, at the missing argument or export.

Batch 321 (257 with the attachments): full waves and a one-lane partial wave.  History 2, net [2 * obs_dim, 16, A] scaled as
tests/test_gpu_actor_softmax.py scales its net (the median spread of the logits is 0.5)."""
import ctypes as C

import numpy as np
import pytest

import _actor_logp_forms as forms
import _actor_logp_twin as ltwin
import _actor_twin as twin
import test_gpu_actor_softmax as soft

pytestmark = pytest.mark.gpu
SEED = soft.SEED
F32 = np.float32
CARTPOLE, MOUNTAINCAR, ACROBOT = soft.CARTPOLE, soft.MOUNTAINCAR, soft.ACROBOT
DIMS = forms.DIMS
N, S = soft.N, soft.S
host = soft.host
_net, _at_the_goal = soft._net, soft._at_the_goal
ACT_SETTINGS = [("uniform", 1.0), ("uniform", 0.5), ("softmax", 0.25), ("softmax", 1.0), ("softmax", 4.0)]
NAN, NEG_INF = np.uint32(ltwin.NAN_BITS), np.array([-np.inf], F32).view(np.uint32)[0]
POISON = forms.POISON


def _u32(t):
    return host(t).view(np.uint32)


def _check_act(env, actor, w, flat, lane0, seed=77, tick=12):
    """Act(logp=) on this handle under every setting and epsilon: actions and logits equal Act's without logp, the action is the softmax
    twin's, logp the logp twin's from the device's own logits"""
    import torch
    n, A = env.NumberOfEnvironments, env.ActionSpace.N
    want_logits, want_greedy = twin.forward(w, flat, actor.History().reshape(n, -1))
    wa, wb = ltwin.words(seed, lane0, tick, n)
    logits, logits0 = (torch.empty((n, A), dtype=torch.float32, device="cuda") for _ in range(2))
    logp = torch.empty(n, dtype=torch.float32, device="cuda")
    out0 = torch.empty(n, dtype=torch.int32, device="cuda")
    for setting in ACT_SETTINGS:
        actor.SetExploration(*setting)
        for eps in (0.0, 0.3, 1.0):
            logits.fill_(-7.0); logits0.fill_(-7.0); logp.fill_(POISON)
            torch.cuda.synchronize()                                     # the fills (torch's stream) end before the handle's stream writes
            plain = host(actor.Act(eps, seed=seed, tick=tick, out=out0, logits=logits0)).copy()
            got = host(actor.Act(eps, seed=seed, tick=tick, logits=logits, logp=logp)).copy()
            assert np.array_equal(got, plain) and np.array_equal(_u32(logits), _u32(logits0))
            assert twin.same(host(logits), want_logits)
            want, want_logp, mask, greedy = ltwin.act_logp(host(logits), wa, wb, eps, *setting)
            assert np.array_equal(greedy, want_greedy)
            assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
            got_logp = _u32(logp).copy()
            print(f"{env.Name} lane0 {lane0} {setting} eps {eps}: explore {int(mask.sum())}/{n}  counts {np.bincount(want, minlength=A).tolist()}  "
                  f"logp mismatches {int((got_logp != want_logp).sum())}  range {want_logp.view(F32).min():.4f} .. {want_logp.view(F32).max():.4f}")
            assert np.array_equal(got_logp, want_logp), np.nonzero(got_logp != want_logp)[0][:8]
            lp = want_logp.view(F32)
            assert np.isfinite(lp).all() and (lp <= 0).all()
            if eps == 1.0 and setting[0] == "softmax":                   # from the twin's side: every action occurs, and logp varies with it
                assert mask.all() and len(np.unique(want)) == A
                g = ltwin.logp(host(logits), greedy, setting[1])
                assert (want_logp != g).any()


@pytest.mark.parametrize("lane0", [0, 5, 2 ** 32 + 6])
@pytest.mark.parametrize("name", [CARTPOLE, MOUNTAINCAR, ACROBOT])
def test_act_with_logp_equals_the_twin(gpu_pkg, name, lane0):
    with gpu_pkg.VectorEnv(name, N, seed=SEED, auto_reset=True, lane_offset=lane0) as env:
        x0 = twin.History(env.Reset(), S).x()
        w, flat, pairs = _net(name, x0)
        actor = env.Actor(pairs, history=S)
        _check_act(env, actor, w, flat, lane0)


def test_act_with_logp_on_a_float64_cartpole_handle(gpu_pkg):
    with gpu_pkg.VectorEnv(CARTPOLE, N, seed=SEED, auto_reset=True, dtype=np.float64) as env:
        x0 = twin.History(np.asarray(env.Reset(), F32), S).x()
        w, flat, pairs = _net(CARTPOLE, x0)
        actor = env.Actor(pairs, history=S)
        _check_act(env, actor, w, flat, 0)


@pytest.mark.parametrize("setting", forms.SETTINGS, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("row", forms.FORMS, ids=forms.form_id)
def test_every_form_equals_single_steps(gpu_pkg, row, setting):
    """T = 12 with max_episode_steps = 5 on the bookkeeping rows, 3 warm steps so that the ring slot is not 0, MountainCar / Acrobot lanes
    put at the goal: the fused rollout with rec_logp equals T x Step(logp=) in rec_logp and in everything the softmax comparison looks at,
    and the poisoned row past T stays poisoned."""
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
    lp = out["logp"].view(F32)
    assert np.isfinite(lp).all() and (lp <= 0).all() and len(np.unique(out["logp"])) > A
    if row["shape"] != "lean":
        assert (out["done"] & 2).any()
    if name != CARTPOLE:
        assert (out["done"][0][np.arange(N) % 3 == 0] & 1).all()


@pytest.mark.parametrize("name", [CARTPOLE, MOUNTAINCAR, ACROBOT])
def test_a_fused_rollout_replays_teacher_forced_through_the_twins(gpu_pkg, name):
    """From the recorded observations and done bytes the history of every step is rebuilt on the host, the fmaf twin gives its logits, and
    the logp twin the log-probability of the RECORDED action: rec_logp, bit for bit (the actions themselves are the softmax twin's)."""
    import torch
    T, eps, tau, aseed, tick0, lane0 = 12, 0.6, 0.5, 99, 1000, 7
    A = DIMS[name][1]
    w, flat, pairs = _net(name)
    with gpu_pkg.VectorEnv(name, N, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=5, lane_offset=lane0) as env:
        obs0 = env.Reset()
        actor = env.Actor(pairs, history=S)
        actor.SetExploration("softmax", tau)
        rec = dict(rec_obs=torch.empty((T, env.ObsDim, N), dtype=torch.float32, device="cuda"), rec_done=torch.empty((T, N), dtype=torch.uint8, device="cuda"),
                   rec_actions=torch.empty((T, N), dtype=torch.int32, device="cuda"), rec_logp=torch.empty((T, N), dtype=torch.float32, device="cuda"))
        env.RolloutFusedDevice(None, T, actions="actor", epsilon=eps, action_seed=aseed, action_tick0=tick0, **rec)
        got = {k: host(v) for k, v in rec.items()}
        model = twin.History(obs0, S)
        for t in range(T):
            logits, _ = twin.forward(w, flat, model.x())
            wa, wb = ltwin.words(aseed, lane0, tick0 + t, N)
            want, want_logp, mask, _ = ltwin.act_logp(logits, wa, wb, eps, "softmax", tau)
            assert np.array_equal(got["rec_actions"][t], want), t
            assert np.array_equal(got["rec_logp"][t].view(np.uint32), want_logp), (t, np.nonzero(got["rec_logp"][t].view(np.uint32) != want_logp)[0][:8])
            model.push(got["rec_obs"][t].T, got["rec_done"][t])
        assert np.array_equal(actor.History(), model.h)
        assert len(np.unique(got["rec_actions"])) == A and (got["rec_done"] & 2).any()


def test_non_finite_logits(gpu_pkg):
    """a last-layer bias of +inf on action 0: 0x7FC00000 on every lane; of -inf on action 1 under uniform exploration at epsilon = 1: -inf
    exactly on the lanes that took action 1, finite elsewhere"""
    import torch
    name, A = ACROBOT, 3
    with gpu_pkg.VectorEnv(name, N, seed=SEED, auto_reset=True) as env:
        env.Reset()
        w, flat, _ = _net(name)
        logp = torch.full((N,), POISON, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        bad = flat.copy()
        bad[-A + 0] = np.inf
        actor = env.Actor(twin.layers(w, bad), history=S)
        for setting in (("uniform", 1.0), ("softmax", 0.5)):
            actor.SetExploration(*setting)
            for eps in (0.0, 1.0):
                actor.Act(eps, seed=3, tick=4, logp=logp)
                assert (_u32(logp) == NAN).all(), (setting, eps)
        bad = flat.copy()
        bad[-A + 1] = -np.inf
        actor = env.Actor(twin.layers(w, bad), history=S)
        logits = torch.empty((N, A), dtype=torch.float32, device="cuda")
        acts = host(actor.Act(1.0, seed=3, tick=4, logits=logits, logp=logp)).copy()
        got = _u32(logp).copy()
        assert (acts == 1).any() and (acts != 1).any()
        assert (got[acts == 1] == NEG_INF).all() and np.isfinite(got[acts != 1].view(F32)).all()
        assert np.array_equal(got, ltwin.logp(host(logits), acts, 1.0))
        actor.SetExploration("softmax", 1.0)                             # ... and the softmax draw never takes it
        acts = host(actor.Act(1.0, seed=3, tick=4, logp=logp)).copy()
        assert not (acts == 1).any() and np.isfinite(_u32(logp).view(F32)).all()


def _spec(capi, T, source, eps=0.5, seed=99, tick0=1000, **rec):
    return capi.RolloutSpec(struct_size=C.sizeof(capi.RolloutSpec), action_source=source, steps=T, action_stride=0, ring=1, action_seed=seed,
                            action_tick0=tick0, epsilon=eps, **{k: C.c_void_p(v.data_ptr()) for k, v in rec.items()})


@pytest.mark.parametrize("setting", [("uniform", 1.0), ("softmax", 0.5)], ids=lambda s: s[0])
def test_the_null_forwarders_equal_the_old_calls(gpu_pkg, setting):
    import importlib
    import torch
    capi = importlib.import_module(gpu_pkg.__name__ + "._capi")
    T = 6
    pairs = _net(CARTPOLE)[2]
    runs = []
    for forwarder in (False, True):
        with gpu_pkg.VectorEnv(CARTPOLE, N, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=5) as env:
            env.Reset()
            lib, h = env._lib, env._h
            actor = env.Actor(pairs, history=S)
            actor.SetExploration(*setting)
            acts = torch.full((N,), -7, dtype=torch.int32, device="cuda")
            logits = torch.full((N, 2), -7.0, dtype=torch.float32, device="cuda")
            rec = dict(d_rec_obs=torch.empty((T, 4, N), dtype=torch.float32, device="cuda"), d_rec_reward=torch.empty((T, N), dtype=torch.float32, device="cuda"),
                       d_rec_done=torch.empty((T, N), dtype=torch.uint8, device="cuda"), d_rec_actions=torch.empty((T, N), dtype=torch.int32, device="cuda"))
            torch.cuda.synchronize()
            name0 = env.KernelName()
            spec = _spec(capi, T, capi.ACTIONS_ACTOR, **rec)
            if forwarder:
                assert lib.gymnet_vecenv_actor_act_logp_device(h, C.c_void_p(acts.data_ptr()), C.c_void_p(logits.data_ptr()), None, C.c_float(0.5), 5, 3) == capi.OK
                assert lib.gymnet_vecenv_rollout_fused_logp_device(h, C.byref(spec), None) == capi.OK
            else:
                assert lib.gymnet_vecenv_actor_act_device(h, C.c_void_p(acts.data_ptr()), C.c_void_p(logits.data_ptr()), C.c_float(0.5), 5, 3) == capi.OK
                assert lib.gymnet_vecenv_rollout_fused_ex_device(h, C.byref(spec)) == capi.OK
            runs.append(dict(kernel=(name0, env.KernelName()), acts=host(acts).copy(), logits=_u32(logits).copy(), state=env.GetState(), hist=actor.History(),
                             tick=env.Tick, done=env.GetArray("done").copy(), ret=env.GetArray("finished_return").copy(),
                             **{k: host(v).copy() for k, v in rec.items()}))
    a, b = runs
    assert a["kernel"] == b["kernel"] and a["tick"] == b["tick"]
    for k in a:
        if k not in ("kernel", "tick"):
            assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k


def test_refusals_write_nothing(gpu_pkg):
    import importlib
    import torch
    capi = importlib.import_module(gpu_pkg.__name__ + "._capi")
    T = 4

    def buffers(n):
        b = dict(acts=torch.full((n,), -7, dtype=torch.int32, device="cuda"), logp=torch.full((n,), POISON, dtype=torch.float32, device="cuda"),
                 rec=torch.full((T, n), POISON, dtype=torch.float32, device="cuda"), rec_act=torch.full((T, n), -7, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        return b

    def intact(b):
        return bool((b["acts"] == -7).all() and (b["logp"] == POISON).all() and (b["rec"] == POISON).all() and (b["rec_act"] == -7).all())

    def act_logp(lib, h, b, eps=0.5):
        return lib.gymnet_vecenv_actor_act_logp_device(h, C.c_void_p(b["acts"].data_ptr()), None, C.c_void_p(b["logp"].data_ptr()), C.c_float(eps), 5, 3)

    def fused_logp(lib, h, b, source, d_actions=None):
        spec = _spec(capi, T, source, d_rec_actions=b["rec_act"])
        if d_actions is not None:
            spec.d_actions = C.c_void_p(d_actions.data_ptr())
        return lib.gymnet_vecenv_rollout_fused_logp_device(h, C.byref(spec), C.c_void_p(b["rec"].data_ptr()))

    with gpu_pkg.VectorEnv("Pendulum-v1", N, seed=SEED) as env:                           # a Box actor
        env.Reset()
        lib, h = env._lib, env._h
        b = buffers(N)
        state, tick = env.GetState(), env.Tick
        assert act_logp(lib, h, b) == capi.ERR_INVALID_ARG                                # no actor
        assert fused_logp(lib, h, b, capi.ACTIONS_ACTOR) == capi.ERR_INVALID_ARG
        actor = env.Actor(twin.net(np.random.default_rng(2), [3, 1])[2], 1)
        hist = actor.History()
        assert act_logp(lib, h, b) == capi.ERR_INVALID_ARG and b"Box" in lib.gymnet_last_error()
        assert fused_logp(lib, h, b, capi.ACTIONS_ACTOR) == capi.ERR_INVALID_ARG and b"Box" in lib.gymnet_last_error()
        assert intact(b) and np.array_equal(env.GetState().view(np.uint32), state.view(np.uint32)) and env.Tick == tick
        assert np.array_equal(actor.History(), hist)
        with pytest.raises(ValueError, match="Box"):
            actor.Act(0.5, 5, 3, logp=b["logp"])
        with pytest.raises(ValueError, match="Box"):
            env.RolloutFusedDevice(None, T, actions="actor", rec_logp=b["rec"])
        actor.Step(0.5, 5, 3)                                                             # the Box actor still works
    with gpu_pkg.VectorEnv(CARTPOLE, N, seed=SEED, auto_reset=True) as env:
        env.Reset()
        lib, h = env._lib, env._h
        b = buffers(N)
        assert act_logp(lib, h, b) == capi.ERR_INVALID_ARG and b"gymnet_vecenv_actor_config" in lib.gymnet_last_error()     # no actor
        assert fused_logp(lib, h, b, capi.ACTIONS_ACTOR) == capi.ERR_INVALID_ARG
        actor = env.Actor(_net(CARTPOLE)[2], history=S)
        ring = torch.zeros((T, N), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        state, tick, hist = env.GetState(), env.Tick, actor.History()
        for source in (capi.ACTIONS_RING, capi.ACTIONS_SAMPLE, capi.ACTIONS_EPSILON_GREEDY, 7):       # d_rec_logp belongs to the actor source
            assert fused_logp(lib, h, b, source, ring) == capi.ERR_INVALID_ARG, source
        assert act_logp(lib, h, b, eps=1.5) == capi.ERR_INVALID_ARG and act_logp(lib, h, b, eps=float("nan")) == capi.ERR_INVALID_ARG
        assert lib.gymnet_vecenv_actor_act_logp_device(h, None, None, C.c_void_p(b["logp"].data_ptr()), C.c_float(0.5), 5, 3) == capi.ERR_INVALID_ARG
        assert lib.gymnet_vecenv_actor_act_logp_device(h, C.c_void_p(b["acts"].data_ptr()), None, C.c_void_p(b["logp"].data_ptr() + 2), C.c_float(0.5), 5, 3) \
            == capi.ERR_INVALID_ARG                                                       # 4-byte alignment
        assert lib.gymnet_vecenv_rollout_fused_logp_device(h, None, C.c_void_p(b["rec"].data_ptr())) == capi.ERR_INVALID_ARG        # a null spec
        spec = _spec(capi, T, capi.ACTIONS_ACTOR, eps=1.5)                                # the rollout's own checks apply
        assert lib.gymnet_vecenv_rollout_fused_logp_device(h, C.byref(spec), C.c_void_p(b["rec"].data_ptr())) == capi.ERR_INVALID_ARG
        spec = _spec(capi, 0, capi.ACTIONS_ACTOR)                                         # steps == 0 writes nothing and is no error
        assert lib.gymnet_vecenv_rollout_fused_logp_device(h, C.byref(spec), C.c_void_p(b["rec"].data_ptr())) == capi.OK
        env.Sync()
        assert intact(b) and np.array_equal(env.GetState().view(np.uint32), state.view(np.uint32)) and env.Tick == tick
        assert np.array_equal(actor.History(), hist)
        # a stale history: one step without a push
        env.StepDevice(actor.Act(0.5, 5, 3))
        state, tick = env.GetState(), env.Tick
        assert act_logp(lib, h, b) == capi.ERR_INVALID_ARG and b"stale" in lib.gymnet_last_error()
        assert fused_logp(lib, h, b, capi.ACTIONS_ACTOR) == capi.ERR_INVALID_ARG and b"stale" in lib.gymnet_last_error()
        env.Sync()
        assert intact(b) and np.array_equal(env.GetState().view(np.uint32), state.view(np.uint32)) and env.Tick == tick
        assert np.array_equal(actor.History(), hist)
        actor.Push()                                                                      # ... and after the push both serve again
        assert act_logp(lib, h, b) == capi.OK
        assert fused_logp(lib, h, b, capi.ACTIONS_RING, ring) == capi.ERR_INVALID_ARG
        rec_act = torch.empty((T, N), dtype=torch.int32, device="cuda")
        plain = dict(actions="actor", epsilon=0.5, action_seed=5, action_tick0=9, rec_actions=rec_act)

        def plain_rollout_leaves_rec_alone():
            env.RolloutFusedDevice(None, T, **plain)
            env.Sync()
            return bool((b["rec"] == POISON).all()) and env.KernelName() == name0

        # the record pointer belongs to the one call that was given it: neither a served nor a refused logp rollout leaves it behind for
        # the plain actor rollout after it to write through
        name0 = env.KernelName()
        assert plain_rollout_leaves_rec_alone()
        env.RolloutFusedDevice(None, T, rec_logp=b["rec"], **plain)
        env.Sync()
        assert not (b["logp"] == POISON).any() and not (b["rec"] == POISON).any()
        b["rec"].fill_(POISON)
        torch.cuda.synchronize()
        assert plain_rollout_leaves_rec_alone()                                           # after a served one
        assert fused_logp(lib, h, b, capi.ACTIONS_RING, ring) == capi.ERR_INVALID_ARG     # refused by the pointer's own checks
        assert plain_rollout_leaves_rec_alone()
        env.StepDevice(actor.Act(0.5, 5, 3))                                              # refused by the rollout's checks, which come after them
        assert fused_logp(lib, h, b, capi.ACTIONS_ACTOR) == capi.ERR_INVALID_ARG and b"stale" in lib.gymnet_last_error()
        actor.Push()
        assert plain_rollout_leaves_rec_alone()
        assert env.Tick == tick + 5 * T + 1
    with gpu_pkg.VectorEnv(CARTPOLE, N, seed=SEED, auto_reset=True, dtype=np.float64) as env:          # float64: act serves, the fused rollout does not
        env.Reset()
        lib, h = env._lib, env._h
        b = buffers(N)
        env.Actor(_net(CARTPOLE)[2], history=S)
        assert fused_logp(lib, h, b, capi.ACTIONS_ACTOR) == capi.ERR_UNSUPPORTED
        env.Sync()
        assert intact(b)


ATT = soft.ATT


def test_actor_step_with_repeat_and_logp_equals_the_unfused_loop(gpu_pkg):
    import torch
    n = 257
    pairs = _net(CARTPOLE, seed=4)[2]
    with gpu_pkg.VectorEnv(CARTPOLE, n, **ATT) as f, gpu_pkg.VectorEnv(CARTPOLE, n, **ATT) as e:
        f.Reset(); e.Reset()
        fa, ea = f.Actor(pairs, history=S), e.Actor(pairs, history=S)
        fa.SetExploration("softmax", 0.5); ea.SetExploration("softmax", 0.5)
        lf, le = (torch.full((n,), POISON, dtype=torch.float32, device="cuda") for _ in range(2))
        logits = torch.empty((n, 2), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        seen = set()
        for d in range(12):
            got = host(fa.Step(0.5, 77, d, repeat=2, logp=lf)).copy()
            want = ea.Act(0.5, 77, d, logits=logits, logp=le)
            e.StepRepeatDevice(want, 2)
            ea.Push()
            assert np.array_equal(got, host(want)), d
            assert np.array_equal(_u32(lf), _u32(le)), d
            assert np.array_equal(_u32(le), ltwin.logp(host(logits), got, 0.5)), d
            seen.update(np.unique(_u32(lf)).tolist())
            assert np.array_equal(f.GetState(), e.GetState()) and f.Tick == e.Tick == 1 + 3 * (d + 1)
            assert np.array_equal(fa.History(), ea.History()), d
        assert len(seen) > 2 and (f.GetArray("finished_length") > 0).any()


def test_memory_rollout_with_rec_logp_equals_single_steps_and_pushes(gpu_pkg):
    import torch
    n, T = 257, 24
    pairs = _net(CARTPOLE, seed=5)[2]
    snaps = []
    for fused in (False, True):
        with gpu_pkg.VectorEnv(CARTPOLE, n, **ATT) as env:
            env.Reset()
            actor = env.Actor(pairs, history=S)
            actor.SetExploration("softmax", 0.5)
            mem = env.EpisodeMemory(capacity=5, max_length=9, history=S, rollout_chunk=16)
            rec = torch.full((T, n), POISON, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            if fused:
                taken = host(mem.Rollout(T, actions="actor", action_seed=77, action_tick0=1000, epsilon=0.5, rec_logp=rec)).copy()
            else:
                rows = []
                for t in range(T):
                    acts = actor.Step(0.5, 77, 1000 + t, logp=rec[t])
                    mem.Push(acts)
                    rows.append(host(acts).copy())
                taken = np.stack(rows)
            x, a, onehot, r = (host(v) for v in mem.BuildDataset("params", min_episodes=0, reward=True))
            snaps.append(dict(taken=taken, logp=_u32(rec).copy(), stats=mem.Stats(), x=x, a=a, onehot=onehot, r=r, state=env.GetState(),
                              hist=actor.History(), tick=env.Tick))
    a, b = snaps
    assert a["stats"] == b["stats"] and a["stats"]["ended"] > 5 and a["tick"] == b["tick"]
    assert np.array_equal(a["taken"], b["taken"]) and len(np.unique(a["taken"])) == 2
    lp = a["logp"].view(F32)
    assert np.isfinite(lp).all() and (lp <= 0).all() and len(np.unique(a["logp"])) > 2
    for k in ("logp", "x", "a", "onehot", "r", "state", "hist"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    with gpu_pkg.VectorEnv(CARTPOLE, n, **ATT) as env:                                    # a ring rollout has no logp to record
        env.Reset()
        env.Actor(pairs, history=S)
        mem = env.EpisodeMemory(capacity=5, max_length=9, history=S, rollout_chunk=16)
        ring = torch.zeros((T, n), dtype=torch.int32, device="cuda")
        tick = env.Tick
        with pytest.raises(ValueError, match="actor"):
            mem.Rollout(T, ring, action_stride=n, ring=T, rec_logp=torch.empty((T, n), dtype=torch.float32, device="cuda"))
        assert mem.Stats()["ended"] == 0 and env.Tick == tick
