"""GPU check of the lifecycle paths the handle's three configurable attachments share (pixel stack, episode memory, actor; their host code
lives beside their kernels in gym.net_amd/csrc/pixel_stack.hip, episode_memory.hip and actor.hip): a re-config with other parameters while
the old attachment is live, a release with the zero argument (the calls are refused again, the other two attachments go on working), a
config after a release, and destroying a handle whose attachments are live.  What a re-configured attachment holds is compared bit for bit
with a second handle that got the second parameter set from the start, at the same state and tick."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 0xA77AC
N = 130                      # two full waves and a ragged third
SIZE = (8, 6)


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _net(rng, widths):
    return [(rng.normal(0, 1, (o, i)).astype(np.float32), rng.normal(0, 1, o).astype(np.float32)) for i, o in zip(widths[:-1], widths[1:])]


def _env(gpu_pkg):
    return gpu_pkg.VectorEnv("CartPole-v1", N, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=8)


CONFIG = {"stack": lambda env, p: env.PixelStack(depth=p["depth"], size=SIZE, format="gray8"),
          "memory": lambda env, p: env.EpisodeMemory(capacity=p["capacity"], max_length=0, history=2),
          "actor": lambda env, p: env.Actor(p["net"], history=p["history"])}
REFUSAL = {"stack": "no pixel stack configured (gymnet_vecenv_pixel_stack_config)",
           "memory": "no episode memory configured (gymnet_vecenv_memory_config)",
           "actor": "no actor configured (gymnet_vecenv_actor_config)"}


def _step(pair, skip=None):
    """One closed-loop vector step on every handle of `pair` (the last one first), every attachment pushed; the first handle has no
    attachment `skip` (without an actor of its own it takes the second handle's actions).  Returns each acting handle's (actions, logits)."""
    import torch
    outs, a = [], None
    for k, (env, att) in reversed(list(enumerate(pair))):
        live = {name: x for name, x in att.items() if not (k == 0 and name == skip)}
        if "actor" in live:
            logits = torch.empty((N, 2), dtype=torch.float32, device="cuda")
            a = live["actor"].Act(epsilon=0.25, seed=11, tick=env.Tick, logits=logits)
            outs.append((_host(a), _host(logits)))
        env.StepDevice(a)
        if "stack" in live:
            live["stack"].Push()
        if "memory" in live:
            live["memory"].Push(a)
        if "actor" in live:
            live["actor"].Push()
    return outs


def _compare(pair, names):
    (ea, a), (eb, b) = pair
    assert _same(ea.GetState(), eb.GetState()) and ea.Tick == eb.Tick
    if "stack" in names:
        assert _same(a["stack"].Read(), b["stack"].Read())
    if "memory" in names:
        assert a["memory"].Stats() == b["memory"].Stats()
        for x, y in zip(a["memory"].Episodes(), b["memory"].Episodes()):
            assert _same(x, y)
        da, db = a["memory"].BuildDataset(min_episodes=0, reward=True), b["memory"].BuildDataset(min_episodes=0, reward=True)
        for x, y in zip(da, db):
            assert _same(_host(x), _host(y))
    if "actor" in names:
        assert _same(a["actor"].History(), b["actor"].History())


def test_reconfig_release_and_destroy_with_live_attachments(gpu_pkg):
    import torch
    E = gpu_pkg._capi
    rng = np.random.default_rng(3)
    first = dict(depth=2, capacity=2, history=2, net=_net(rng, [8, 4, 2]))
    second = dict(depth=3, capacity=3, history=1, net=_net(rng, [4, 4, 2]))
    with _env(gpu_pkg) as env, _env(gpu_pkg) as ref:
        env.Reset()
        s = np.zeros((4, N), np.float32)          # lanes close to the thresholds, episodes of every age: some end in every step
        s[0], s[1] = rng.uniform(-2.3, 2.3, N), rng.uniform(-1, 1, N)
        s[2], s[3] = rng.uniform(-0.2, 0.2, N), rng.uniform(-1.5, 1.5, N)
        env.SetState(s)
        env.SetArray("episode_length", rng.integers(0, 8, N).astype(np.int32))
        att = {name: CONFIG[name](env, first) for name in CONFIG}
        for _ in range(3):
            _step([(env, att)])
        assert att["memory"].Stats()["ended"] > 0
        att = {name: CONFIG[name](env, second) for name in CONFIG}           # re-config over the live attachments
        ref.Reset()
        ref.Restore(env.Checkpoint())                                      # state, tick, running episode lengths and returns
        ratt = {name: CONFIG[name](ref, second) for name in CONFIG}
        pair = [(env, att), (ref, ratt)]
        for _ in range(3):
            (ra, rl), (a, l) = _step(pair)
            assert _same(a, ra) and _same(l, rl)
        st = att["memory"].Stats()
        assert st["ended"] > 0 and st["kept"] == 3
        _compare(pair, ("stack", "memory", "actor"))

        lib, h = env._lib, env._h
        buf = torch.zeros(N, dtype=torch.int32, device="cuda")
        p, v = C.c_void_p(buf.data_ptr()), [C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int32()]
        release = {"stack": lambda: lib.gymnet_vecenv_pixel_stack_config(h, 0, 0, 0, 0, 0, 0, 0, 0, None, 0),
                   "memory": lambda: lib.gymnet_vecenv_memory_config(h, 0, 0, 0),
                   "actor": lambda: lib.gymnet_vecenv_actor_config(h, 0, 0, None, None, 0)}
        refused = {"stack": [lambda: lib.gymnet_vecenv_pixel_stack_push_device(h, None),
                             lambda: lib.gymnet_vecenv_pixel_stack_view(h, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]))],
                   "memory": [lambda: lib.gymnet_vecenv_memory_push_device(h, p, None)],
                   "actor": [lambda: lib.gymnet_vecenv_actor_push_device(h, None),
                             lambda: lib.gymnet_vecenv_actor_view(h, C.byref(v[0]), C.byref(v[1]), C.byref(v[3])),
                             lambda: lib.gymnet_vecenv_actor_act_device(h, p, None, 0.0, 0, 0)]}
        for name in ("stack", "memory", "actor"):
            assert release[name]() == 0
            for call in refused[name]:
                assert call() == E.ERR_INVALID_ARG and REFUSAL[name] in E.last_error()
            _step(pair, skip=name)                                         # the other two go on working
            _compare(pair, [x for x in CONFIG if x != name])
            att[name], ratt[name] = CONFIG[name](env, second), CONFIG[name](ref, second)      # a config after a release
        (ra, rl), (a, l) = _step(pair)
        assert _same(a, ra) and _same(l, rl)
        _compare(pair, ("stack", "memory", "actor"))
    # both handles were destroyed with their three attachments live
