"""GPU checks of the episode memory's rollout ingest (gymnet_vecenv_memory_config_rollout / _push_rollout_device; EpisodeMemory.PushRollout
and .Rollout) against the path it replaces, on twin handles with the same seed: handle A runs T x (StepDevice, mem.Push), handle B one fused
rollout that records observations, rewards, done bytes and actions, then one PushRollout.  Both go on with 3 single steps, a second
ingest of C + 1 steps, a masked reset of handle and memory and 13 more single steps, each after a masked reset of the memory alone (the
lanes it opens end episodes of a few rows: on Acrobot, whose return is minus the length, only those evict); after every stage Stats(), Episodes() and the
params dataset (CartPole float32: the binary8 pixel dataset too) are compared bit for bit.

The shapes are the smallest that reach every path: 300 lanes (two workgroups, a last wave of 44 lanes), max_episode_steps 12 with
max_length 10 (11- and 12-step episodes are too long), 5 kept episodes, T = 70 steps in passes of C = 16 (four full passes and one of 6;
T > L + C: the staging ring wraps several times).  Before the memory is configured the lanes' episode clocks are staggered by masked
resets, so that the first episodes the memory sees end in different steps with 1 .. 12 rows — also on Pendulum and Acrobot, whose
episodes only end by truncation.  Every twin case asserts from handle A's sequential stats that the pool overflowed, evicted and met
episodes that were too long, and that one pass saw episodes end in two different steps."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 0x5EED
K, L, MAX_STEPS, T, HISTORY = 5, 10, 12, 70, 2
PRELUDE, TAIL = 11, 13
ENVS = [("CartPole-v1", np.float32), ("CartPole-v1", np.float64), ("Pendulum-v1", np.float32), ("Acrobot-v1", np.float32)]
CHUNKS = [0, 1, 2, 16, 64]              # 0: the plain EpisodeMemory(...) config, which ingests one step per pass
# the one-lane case needs short episodes to overflow a pool of 5 in 100 steps: its actions repeat (STICKY), and its seed is one for
# which the assertions of _not_vacuous hold
ONE_LANE_SEED = 1
STICKY = 0.9


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _actions(env, rng, rows, sticky=0.0):
    """[rows][N] random actions: uniform in the Box bounds, or uniform over the Discrete values — with probability `sticky` replaced by
    the value the lane took in row 0"""
    n = env.NumberOfEnvironments
    if env._adtype == np.float32:
        return rng.uniform(env._info.action_low, env._info.action_high, (rows, n)).astype(np.float32)
    a = rng.integers(0, env.ActionSpace.N, (rows, n)).astype(np.int32)
    return np.where(rng.random((rows, n)) < sticky, a[0], a).astype(np.int32)


def _snapshot(env, mem):
    """every observable of the memory, as host arrays"""
    out = {"stats": mem.Stats(), "episodes": mem.Episodes(), "rows": mem.DatasetSize()}
    formats = ["params"] + (["binary8"] if env.Name.startswith("CartPole") and env.Dtype == np.float32 else [])
    for f in formats:
        got = mem.BuildDataset(f, min_episodes=0, reward=True)
        out[f] = [None if v is None else v.cpu().numpy() for v in got]
    return out


def _same(a, b, what):
    assert a["stats"] == b["stats"], (what, a["stats"], b["stats"])
    assert a["rows"] == b["rows"], what
    for x, y, name in zip(a["episodes"], b["episodes"], ("return", "length", "end_tick", "lane")):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, name)
    for f in ("params", "binary8"):
        assert (f in a) == (f in b)
        for x, y in zip(a.get(f, []), b.get(f, [])):
            assert (x is None) == (y is None), (what, f)
            if x is not None:
                assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, f)


def _rec(env, steps):
    import torch
    n = env.NumberOfEnvironments
    return (torch.empty((steps, env.ObsDim, n), dtype=getattr(torch, env.Dtype.name), device="cuda"),
            torch.empty((steps, n), dtype=torch.float32, device="cuda"), torch.empty((steps, n), dtype=torch.uint8, device="cuda"))


def _reset_done_lanes(env, mem):
    """without auto-reset: the lanes that finished are reset and opened again"""
    mask = _dev((env.GetArray("done") != 0).astype(np.uint8))
    env.ResetWhereDevice(mask)
    mem.Reset(mask)


def _scenario(pkg, env_name, dtype, auto_reset, n, chunk, t2, fused, seed=0, sticky=0.0):
    """the stages on one handle; fused: the two ingests (T and t2 steps) go through RolloutFusedDevice + PushRollout, else through
    single steps and pushes.  Returns the snapshots after every stage and the done rows of the two ingested launches."""
    with pkg.VectorEnv(env_name, n, seed=SEED, auto_reset=auto_reset, episode_stats=True, max_episode_steps=MAX_STEPS, dtype=dtype) as env:
        rng = np.random.default_rng(seed)
        env.Reset()
        pre, a1, a3, a2, a4 = (_dev(_actions(env, rng, r, sticky)) for r in (PRELUDE, T, 3, t2, TAIL))
        for i in range(PRELUDE):                   # lane k's episode clock ends up at 10 - k % 12 (k % 12 == 11: 11)
            env.StepDevice(pre[i])
            env.ResetWhereDevice(_dev((np.arange(n) % 12 == i).astype(np.uint8)))
        mem = env.EpisodeMemory(capacity=K, max_length=L, history=HISTORY, rollout_chunk=chunk)
        snaps, done_rows = [], []

        def ingest(actions, steps):
            if fused:
                obs, rew, done = _rec(env, steps)
                env.RolloutFusedDevice(actions, steps, n, steps, rec_obs=obs, rec_reward=rew, rec_done=done)
                mem.PushRollout(steps, obs, actions, rew, done, action_stride=n, ring=steps)
                env.Sync()
                done_rows.append(done.cpu().numpy())
            else:
                rows = []
                for t in range(steps):
                    env.StepDevice(actions[t])
                    mem.Push(actions[t])
                    rows.append(env.GetArray("done"))
                done_rows.append(np.stack(rows))
            snaps.append(_snapshot(env, mem))

        def singles(actions, reopen=False):
            for t in range(actions.shape[0]):
                if reopen:                         # lanes k % 13 == t abandon their partial episode: short episodes late in the run
                    mem.Reset(_dev((np.arange(n) % 13 == t).astype(np.uint8)))
                env.StepDevice(actions[t])
                mem.Push(actions[t])
            snaps.append(_snapshot(env, mem))

        ingest(a1, T)
        if not auto_reset:
            _reset_done_lanes(env, mem)
        singles(a3)
        if not auto_reset:
            _reset_done_lanes(env, mem)
        ingest(a2, t2)
        mask = _dev((np.arange(n) % 3 == 0).astype(np.uint8))
        env.ResetWhereDevice(mask)
        mem.Reset(mask)
        singles(a4, reopen=True)
        return snaps, done_rows


@functools.lru_cache(maxsize=None)
def _sequential(pkg, env_name, dtype, auto_reset, n, t2, seed, sticky):
    """handle A of a case, a memory from the plain config: computed once for every chunk size that shares its second ingest's length"""
    return _scenario(pkg, env_name, dtype, auto_reset, n, 0, t2, False, seed, sticky)


def _not_vacuous(snaps, done_rows, chunk):
    st = snaps[-1]["stats"]
    assert st["ended"] > K and st["admitted"] > st["kept"] and st["too_long"] > 0, st
    if max(chunk, 1) > 1:                          # one pass saw episodes end in two of its steps
        c = max(chunk, 1)
        assert any(done_rows[0][t0:t0 + c].any(axis=1).sum() >= 2 for t0 in range(0, T, c))


def _twins(pkg, env_name, dtype, auto_reset, n, chunk, seed=0, sticky=0.0):
    a_snaps, a_done = _sequential(pkg, env_name, dtype, auto_reset, n, max(chunk, 1) + 1, seed, sticky)
    b_snaps, b_done = _scenario(pkg, env_name, dtype, auto_reset, n, chunk, max(chunk, 1) + 1, True, seed, sticky)
    _not_vacuous(a_snaps, a_done, chunk)
    for x, y in zip(a_done, b_done):
        assert np.array_equal(x, y)
    for i, (x, y) in enumerate(zip(a_snaps, b_snaps)):
        _same(x, y, f"stage {i}")


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("auto_reset", [True, False])
@pytest.mark.parametrize("env_name,dtype", ENVS)
def test_ingest_equals_single_pushes(gpu_pkg, env_name, dtype, auto_reset, chunk):
    _twins(gpu_pkg, env_name, dtype, auto_reset, 300, chunk)


# (one lane without auto-reset ends three episodes in the whole scenario: it cannot overflow a pool of 5)
@pytest.mark.parametrize("n,auto_reset,chunk,seed,sticky", [(1, True, 16, ONE_LANE_SEED, STICKY), (1, True, 0, ONE_LANE_SEED, STICKY),
                                                            (64, True, 16, 0, 0.0), (64, True, 0, 0, 0.0), (64, False, 16, 0, 0.0),
                                                            (64, False, 1, 0, 0.0)])
def test_ingest_equals_single_pushes_at_other_batch_sizes(gpu_pkg, n, auto_reset, chunk, seed, sticky):
    _twins(gpu_pkg, "CartPole-v1", np.float32, auto_reset, n, chunk, seed, sticky)


# ---- every action source of the fused rollout ----------------------------------------------------------------------------------------
ASEED, ATICK0, EPS = 77, 1000, 0.3


def _net(rng, widths):
    return [((rng.standard_normal((o, i)) * 0.7).astype(np.float32), (rng.standard_normal(o) * 0.1).astype(np.float32))
            for i, o in zip(widths[:-1], widths[1:])]


def _source_pair(pkg, source, via_rollout=False):
    """(snapshot of the sequential handle, snapshot of the fused one, sequential stats) for one action source"""
    import torch
    n = 300
    env_name = "Pendulum-v1" if source == "box_actor" else "CartPole-v1"
    rng = np.random.default_rng(11)
    net = _net(rng, [HISTORY * 3, 8, 1] if source == "box_actor" else [HISTORY * 4, 8, 2])
    policy = rng.integers(0, 2, (4 if source == "ring4" else T, n)).astype(np.int32)
    repeat = 2 if source == "repeat" else 0
    out = []
    for fused in (False, True):
        with pkg.VectorEnv(env_name, n, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=MAX_STEPS) as env:
            env.Reset()
            ring = _dev(policy)
            actor = None
            if source in ("actor", "box_actor"):
                actor = env.Actor(net, history=HISTORY)
                if source == "box_actor":
                    actor.SetPolicy("tanh", "gaussian", 0.5)
            mem = env.EpisodeMemory(capacity=K, max_length=MAX_STEPS, history=HISTORY, rollout_chunk=16)
            if not fused:
                a = torch.empty(n, dtype=torch.int32, device="cuda")
                for t in range(T):
                    if source in ("ring", "ring4", "repeat"):
                        mem.Step(ring[t % ring.shape[0]], repeat=repeat)
                    elif source == "sample":
                        env.SampleActionsDevice(a, seed=ASEED, tick=ATICK0 + t)
                        mem.Step(a)
                    elif source == "epsilon_greedy":
                        env.ComposeActionsDevice(ring[t], EPS, a, seed=ASEED, tick=ATICK0 + t)
                        mem.Step(a)
                    else:
                        mem.Push(actor.Step(EPS, ASEED, ATICK0 + t))
            else:
                kw = {}
                if source in ("ring", "ring4", "repeat"):
                    kw = dict(action_stride=n, ring=ring.shape[0], repeat=repeat)
                elif source == "sample":
                    kw = dict(actions="sample", action_seed=ASEED, action_tick0=ATICK0)
                elif source == "epsilon_greedy":
                    kw = dict(actions="epsilon_greedy", action_stride=n, ring=T, action_seed=ASEED, action_tick0=ATICK0, epsilon=EPS)
                else:
                    kw = dict(actions="actor", action_seed=ASEED, action_tick0=ATICK0, epsilon=EPS)
                d_actions = None if source in ("sample", "actor", "box_actor") else ring
                if via_rollout:
                    mem.Rollout(T, d_actions, **kw)
                else:
                    obs, rew, done = _rec(env, T)
                    if source in ("ring", "ring4", "repeat"):
                        env.RolloutFusedDevice(d_actions, T, rec_obs=obs, rec_reward=rew, rec_done=done, **kw)
                        mem.PushRollout(T, obs, ring, rew, done, action_stride=n, ring=ring.shape[0])      # the ring, verbatim
                    else:
                        act = torch.empty((T, n), dtype=torch.float32 if source == "box_actor" else torch.int32, device="cuda")
                        env.RolloutFusedDevice(d_actions, T, rec_obs=obs, rec_reward=rew, rec_done=done, rec_actions=act, **kw)
                        mem.PushRollout(T, obs, act, rew, done)
            snap = _snapshot(env, mem)
            # the memory goes on as after single pushes: a few more of them, and the actor's history is current too
            a = _dev(_actions(env, np.random.default_rng(5), 13))
            for t in range(13):
                mem.Step(a[t])
                if actor:
                    actor.Push()
            out.append((snap, _snapshot(env, mem), env.Tick))
    return out


@pytest.mark.parametrize("source", ["ring", "ring4", "sample", "epsilon_greedy", "actor", "box_actor", "repeat"])
def test_every_action_source_and_frame_skip(gpu_pkg, source):
    (a0, a1, a_tick), (b0, b1, b_tick) = _source_pair(gpu_pkg, source)
    assert a0["stats"]["ended"] > K and a0["stats"]["kept"] == K and a0["stats"]["admitted"] > K      # (max_length = the time limit here)
    _same(a0, b0, source)
    _same(a1, b1, source + " (later pushes)")
    assert a_tick == b_tick == 1 + (3 if source == "repeat" else 1) * T + 13
    if source == "repeat":                         # end ticks on the engine clock: a decision is 3 ticks
        assert ((a0["episodes"][2] - 1) % 3 == 0).all() and np.array_equal(a0["episodes"][2], b0["episodes"][2])


@pytest.mark.parametrize("source", ["ring4", "sample"])
def test_rollout_equals_the_two_calls_it_wraps(gpu_pkg, source):
    (a0, a1, _), (b0, b1, _) = _source_pair(gpu_pkg, source, via_rollout=True)
    _same(a0, b0, source)
    _same(a1, b1, source + " (later pushes)")


def test_rollout_returns_the_actions_taken_and_reuses_its_buffers(gpu_pkg):
    import torch
    n = 64
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=MAX_STEPS) as env:
        env.Reset()
        mem = env.EpisodeMemory(capacity=K, max_length=L, history=HISTORY, rollout_chunk=4)
        got = mem.Rollout(9, actions="sample", action_seed=ASEED, action_tick0=ATICK0)
        want = torch.empty(n, dtype=torch.int32, device="cuda")
        env.SampleActionsDevice(want, seed=ASEED, tick=ATICK0 + 8)
        env.Sync()
        assert tuple(got.shape) == (9, n) and torch.equal(got[8], want)
        assert mem.Rollout(9, actions="sample", action_seed=ASEED, action_tick0=ATICK0 + 9).data_ptr() == got.data_ptr()
        ring = _dev(np.zeros((2, n), np.int32))
        assert mem.Rollout(5, ring, action_stride=n, ring=2) is ring
        with pytest.raises(TypeError):
            mem.Rollout(5, ring, rec_obs=None)


# ---- refusals and lifetime ---------------------------------------------------------------------------------------------------------------
def test_refused_ingests_write_nothing(gpu_pkg):
    n, steps = 300, 20
    inv = gpu_pkg._capi.ERR_INVALID_ARG
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=MAX_STEPS) as env:
        env.Reset()
        lib, h = env._lib, env._h
        ring = _dev(np.random.default_rng(2).integers(0, 2, (steps, n)).astype(np.int32))
        obs, rew, done = _rec(env, steps)
        p = lambda t: C.c_void_p(t.data_ptr())
        push = lambda s, o=obs, a=ring, r=rew, d=done, stride=n, rg=steps: lib.gymnet_vecenv_memory_push_rollout_device(
            h, s, None if o is None else p(o), None if a is None else p(a), stride, rg, None if r is None else p(r), None if d is None else p(d))
        assert push(steps) == inv and b"no episode memory" in lib.gymnet_last_error()
        for bad in (65, -1):
            assert lib.gymnet_vecenv_memory_config_rollout(h, K, L, HISTORY, bad) == inv
            with pytest.raises(ValueError):
                env.EpisodeMemory(K, L, HISTORY, rollout_chunk=bad)
        assert push(steps) == inv and b"no episode memory" in lib.gymnet_last_error()      # a refused config configures nothing
        mem = env.EpisodeMemory(capacity=K, max_length=L, history=HISTORY, rollout_chunk=16)
        env.RolloutFusedDevice(ring, steps, n, steps, rec_obs=obs, rec_reward=rew, rec_done=done)
        mem.PushRollout(steps, obs, ring, rew, done)
        before = _snapshot(env, mem)
        assert before["stats"]["ended"] > 0

        def unchanged():
            _same(before, _snapshot(env, mem), "after a refusal")

        assert push(steps) == inv and b"exactly one" in lib.gymnet_last_error()            # a second ingest, no launch in between
        unchanged()
        env.RolloutFusedDevice(ring, steps, n, steps, rec_obs=obs, rec_reward=rew, rec_done=done)
        for s in (steps - 1, steps + 1, 0, -3):
            assert push(s) == inv
        assert b"seen" in lib.gymnet_last_error() or b"steps" in lib.gymnet_last_error()
        assert push(steps - 1) == inv and (b"%d step(s) seen, %d asked" % (steps, steps - 1)) in lib.gymnet_last_error()
        for kw in (dict(o=None), dict(a=None), dict(r=None), dict(d=None), dict(rg=0), dict(stride=-1)):
            assert push(steps, **kw) == inv, kw
        assert lib.gymnet_vecenv_memory_push_device(h, p(ring), None) == inv               # the single push still refuses a rollout
        assert b"exactly one" in lib.gymnet_last_error()
        unchanged()
        mem.PushRollout(steps, obs, ring, rew, done)                                       # the matching ingest is still accepted
        before = _snapshot(env, mem)
        env.Reset()                                                                        # a handle reset without a memory reset
        env.RolloutFusedDevice(ring, steps, n, steps, rec_obs=obs, rec_reward=rew, rec_done=done)
        assert push(steps) == inv
        unchanged()
        mem.Reset()
        env.RolloutFusedDevice(ring, 3, n, steps, rec_obs=obs, rec_reward=rew, rec_done=done, repeat=1)
        env.Tick = env.Tick + 1                        # 4 decision ticks in one launch, but 7 engine ticks: no launch of 4 decisions
        assert push(4) == inv and b"not one launch" in lib.gymnet_last_error()
        unchanged()
        mem.Reset()
        env.RolloutFusedDevice(ring, steps, n, steps, rec_obs=obs, rec_reward=rew, rec_done=done)
        mem.PushRollout(steps, obs, ring, rew, done)                                       # after the memory reset it is accepted again
        assert mem.Stats()["ended"] > before["stats"]["ended"]
        for bad in (dict(steps=0), dict(steps=True), dict(steps=2.0), dict(ring=0), dict(action_stride=-1)):
            kw = dict(steps=steps, ring=None, action_stride=None)
            kw.update(bad)
            with pytest.raises(ValueError):
                mem.PushRollout(kw.pop("steps"), obs, ring, rew, done, **kw)


def _obs_soa(env):
    """the handle's current observations as the rollout records them: [obs_dim][N]"""
    import torch
    n = env.NumberOfEnvironments
    rowmajor = torch.empty((n, env.ObsDim), dtype=getattr(torch, env.Dtype.name), device="cuda")
    env.PackObsDevice(rowmajor)
    env.Sync()
    return rowmajor.cpu().numpy().T


def test_a_single_step_ingests_with_steps_1(gpu_pkg):
    n = 300
    rng = np.random.default_rng(8)
    snaps = []
    for fused in (False, True):
        with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=MAX_STEPS) as env:
            env.Reset()
            a = _dev(np.random.default_rng(8).integers(0, 2, (30, n)).astype(np.int32))
            mem = env.EpisodeMemory(capacity=K, max_length=L, history=HISTORY, rollout_chunk=0 if fused else 4)
            for t in range(30):
                env.StepDevice(a[t])
                if fused:
                    mem.PushRollout(1, _dev(_obs_soa(env)), a[t], _dev(env.GetArray("reward")), _dev(env.GetArray("done")))
                else:
                    mem.Push(a[t])
            snaps.append(_snapshot(env, mem))
    assert snaps[0]["stats"]["ended"] > K
    _same(snaps[0], snaps[1], "steps = 1")


def test_reconfig_replaces_the_memory_and_close_releases_it(gpu_pkg):
    n, steps = 64, 8
    inv = gpu_pkg._capi.ERR_INVALID_ARG
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=MAX_STEPS) as env:
        env.Reset()
        ring = _dev(np.random.default_rng(1).integers(0, 2, (steps, n)).astype(np.int32))
        first = env.EpisodeMemory(capacity=K, max_length=L, history=HISTORY, rollout_chunk=8)
        first.Rollout(steps, ring, action_stride=n, ring=steps)
        for chunk in (0, 3):                       # either config call replaces it, with an empty pool
            mem = env.EpisodeMemory(capacity=K, max_length=L, history=HISTORY, rollout_chunk=chunk)
            assert mem.RolloutChunk == chunk and mem.Stats() == {"kept": 0, "ended": 0, "admitted": 0, "too_long": 0}
            with pytest.raises(ValueError):
                first.Stats()
            mem.Rollout(2 * steps, ring, action_stride=n, ring=steps)
            assert mem.Stats()["ended"] > 0
            first = mem
        mem.Close()
        assert env._lib.gymnet_vecenv_memory_push_rollout_device(env._h, 1, None, None, 0, 1, None, None) == inv
        assert b"no episode memory" in env._lib.gymnet_last_error()
        with pytest.raises(ValueError):
            mem.Rollout(steps, ring, action_stride=n, ring=steps)
