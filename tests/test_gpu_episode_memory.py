"""GPU checks of the episode memory (gym.net_amd/csrc/episode_memory.hip, gymnet_vecenv_memory_*) against the NumPy model
(tests/_episode_memory_model.py) fed with what the step API returned: the kept set (return, length, end tick, lane) after every push
for small batches and at the end for large ones, in CartPole float32 / float64, a Box-action env and Acrobot; returns bit-equal to the
EPISODE_STATS finished returns; params datasets bit for bit; pixel datasets equal to the PixelStack captured when each action was
chosen; handles without auto-reset with masked resets and closed lanes; too_long and clear_pool; refused pushes write nothing; a twin
handle without a memory stays bit-identical.  The edges, against the same model: episodes of up to 200 rows in a ring that wraps twice
(more than one 64-row trip of the merge's copy, dataset rows beyond a block's 64th, params and pixel datasets), 256 candidates of 150
rows in one push, end ticks that cross 2^32 (the tick digits of the radix select), a dataset call with capacity_rows below the dataset's
rows, and pushes that get the caller's own done bytes."""
import ctypes as C

import numpy as np
import pytest

import _episode_memory_model as model
import _pixel_stack_model as stack_model

pytestmark = pytest.mark.gpu
SEED = 0x5EED


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _actions(env, rng, t, obs=None):
    if env._adtype == np.float32:                                         # Box (Pendulum / MountainCarContinuous)
        lo, hi = env._info.action_low, env._info.action_high
        return rng.uniform(lo, hi, env.NumberOfEnvironments).astype(np.float32)
    return model.mixed_policy(env.NumberOfEnvironments, rng, t, env.ActionSpace.N)     # an epsilon-greedy mix of a fixed policy and samples


def _check_kept(mem, m):
    got = mem.Episodes()
    want = m.kept()
    for g, w, name in zip(got, want, ("return", "length", "end_tick", "lane")):
        assert np.array_equal(g, w), name
    st = mem.Stats()
    assert (st["kept"], st["ended"], st["too_long"], st["admitted"]) == (len(m.pool), m.ended, m.too_long, m.admitted)


def _loop(gpu_pkg, env_name, n, capacity, steps, every_push, dtype=np.float32, max_steps=60, max_length=0, history=4, then=None,
          policy=_actions, start_tick=None, own_done=0.0, after_push=None):
    """policy(env, rng, t, obs): the actions of step t from the last returned observations; start_tick: set before the memory is
    configured; own_done: the push gets the caller's done bytes, the handle's OR a mask of that density, and so does the model;
    after_push(m, t): called after every push."""
    rng = np.random.default_rng(n + capacity)
    with gpu_pkg.VectorEnv(env_name, n, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=max_steps, dtype=dtype) as env:
        obs = env.Reset()
        if start_tick is not None:
            env.Tick = start_tick
        mem = env.EpisodeMemory(capacity=capacity, max_length=max_length, history=history)
        m = model.EpisodeMemoryModel(obs, capacity, max_length or max_steps, history)
        for t in range(steps):
            a = policy(env, rng, t, obs)
            out = env.Step(a)
            obs = out.Observation
            d = out.Done.astype(np.uint8)
            if own_done:
                d |= (rng.random(n) < own_done).astype(np.uint8)
                mem.Push(_dev(a), done=_dev(d))
            else:
                mem.Push(_dev(a))
            ended = m.push(a, out.Reward, d, out.Observation, env.Tick)
            if d.any() and not own_done:                                  # the memory's returns are the EPISODE_STATS ones, bit for bit
                fin = env.GetArray("finished_return")
                lanes = [e["lane"] for e in ended]
                assert np.array_equal(fin[lanes].view(np.uint32), np.array([e["ret"] for e in ended], np.float32).view(np.uint32))
            if every_push:
                _check_kept(mem, m)
            if after_push:
                after_push(m, t)
        _check_kept(mem, m)
        rows = _params_dataset(env, mem, m)
        if then:
            then(env, mem, m)
        return m, rows


def _params_dataset(env, mem, m):
    action_n = None if env._adtype == np.float32 else env.ActionSpace.N
    x, a, oh, r = m.dataset_params(action_n)
    got = mem.BuildDataset("params", min_episodes=0, reward=True)
    assert mem.DatasetSize() == len(x)
    gx, ga, goh, gr = (None if v is None else v.cpu().numpy() for v in got)
    assert np.array_equal(gx, x) and np.array_equal(gr, r)
    assert np.array_equal(ga.view(np.uint32), a.astype(ga.dtype).view(np.uint32))
    if action_n:
        assert np.array_equal(goh, oh)
    else:
        assert goh is None
    return len(x)


@pytest.mark.parametrize("capacity,n,steps", [(1, 1 << 10, 120), (100, 1 << 10, 150), (4096, 1 << 12, 120)])
def test_cartpole_kept_set_equals_the_model_after_every_push(gpu_pkg, capacity, n, steps):
    m, rows = _loop(gpu_pkg, "CartPole-v1", n, capacity, steps, every_push=True)
    assert len(m.pool) == min(capacity, m.ended) and rows > 0


def test_cartpole_large_batch_matches_the_model_at_the_end(gpu_pkg):
    m, _ = _loop(gpu_pkg, "CartPole-v1", 1 << 16, 100, 80, every_push=False)
    assert m.ended > 10000 and m.admitted > 100


@pytest.mark.parametrize("env_name,dtype", [("CartPole-v1", np.float64), ("Pendulum-v1", np.float32), ("Acrobot-v1", np.float32),
                                            ("MountainCarContinuous-v0", np.float32)])
def test_other_dtypes_box_actions_and_obs_dims(gpu_pkg, env_name, dtype):
    m, rows = _loop(gpu_pkg, env_name, 512, 50, 90, every_push=True, dtype=dtype, max_steps=25, history=3)
    assert m.ended > 0 and rows > 0


def test_too_long_and_clear_pool(gpu_pkg):
    def clear(env, mem, m):
        mem.Reset(clear=True)
        assert mem.Stats() == {"kept": 0, "ended": 0, "admitted": 0, "too_long": 0}
        assert mem.BuildDataset("params") is None and mem.DatasetSize() == 0
    m, _ = _loop(gpu_pkg, "CartPole-v1", 1024, 64, 100, every_push=True, max_steps=40, max_length=12, then=clear)
    assert m.too_long > 0 and (np.array([e["len"] for e in m.pool]) <= 12).all()


def test_without_autoreset_masked_resets_and_closed_lanes(gpu_pkg):
    n, capacity = 777, 40
    rng = np.random.default_rng(3)
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=False) as env:
        obs = env.Reset()
        mem = env.EpisodeMemory(capacity=capacity, max_length=200, history=2)
        m = model.EpisodeMemoryModel(obs, capacity, 200, 2, autoreset=False)
        done_ever = np.zeros(n, bool)
        for t in range(120):
            a = rng.integers(0, 2, n).astype(np.int32)
            out = env.Step(a)
            mem.Push(_dev(a))
            m.push(a, out.Reward, out.Done.astype(np.uint8), out.Observation, env.Tick)
            done_ever |= out.Done
            if t % 15 == 14:                                              # reset half of the finished lanes
                mask = (done_ever & (rng.random(n) < 0.5)).astype(np.uint8)
                obs = env.ResetWhere(mask)
                mem.Reset(_dev(mask))
                m.reset(obs, mask)
                done_ever &= mask == 0
            _check_kept(mem, m)
        _params_dataset(env, mem, m)


def test_pixel_datasets_equal_the_pixel_stack_at_action_time(gpu_pkg):
    import torch
    n, capacity, depth, steps = 256, 24, 2, 70
    crop, size = (200, 150, 200, 150), (40, 20)
    rng = np.random.default_rng(9)
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=40) as env:
        obs0 = env.Reset()
        stack = env.PixelStack(depth=depth, size=size, crop=crop, format="gray8")
        mem = env.EpisodeMemory(capacity=capacity, max_length=0, history=depth)
        m = model.EpisodeMemoryModel(obs0, capacity, 40, depth)
        seen = []                                                         # history index t -> the stacks when step t's action was chosen
        for t in range(steps):
            env.Sync()
            seen.append(stack.Tensor.cpu().numpy())
            a = _actions(env, rng, t)
            d_a = _dev(a)
            env.StepDevice(d_a)
            stack.Push()
            mem.Push(d_a)
            env.Sync()
            done = env.GetArray("done")
            m.push(a, env.GetArray("reward"), done, env.GetState().T.copy(), env.Tick)
        _check_kept(mem, m)
        rows = m.dataset_rows()
        assert len(rows) > 0
        gray = np.stack([seen[e["start"] + p][e["lane"]] for e, p, _ in rows])
        for fmt in ("gray8", "binary8", "binary_f32"):
            x, a, oh = mem.BuildDataset(fmt, size=size, crop=crop, min_episodes=capacity)
            want = stack_model.process(gray, {"gray8": 2, "binary8": 3, "binary_f32": 4}[fmt])
            assert np.array_equal(x.cpu().numpy(), want), fmt
            assert x.dtype == (torch.float32 if fmt == "binary_f32" else torch.uint8)
        assert env._lib.gymnet_vecenv_memory_dataset_device(env._h, 2, 0, 0, 700, 10, 40, 20, None, None, None, None, 1) != 0


def test_refused_calls_write_nothing_and_a_twin_stays_identical(gpu_pkg):
    import torch
    n = 2048
    rng = np.random.default_rng(11)
    kw = dict(seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=30)
    with gpu_pkg.VectorEnv("CartPole-v1", n, **kw) as env, gpu_pkg.VectorEnv("CartPole-v1", n, **kw) as twin:
        env.Reset(); twin.Reset()
        mem = env.EpisodeMemory(capacity=32, history=4)
        lib, h = env._lib, env._h
        inv = gpu_pkg._capi.ERR_INVALID_ARG
        for t in range(60):
            a = rng.integers(0, 2, n).astype(np.int32)
            o1, o2 = env.Step(a), twin.Step(a)
            mem.Push(_dev(a))
            assert np.array_equal(o1.Observation, o2.Observation) and np.array_equal(o1.Reward, o2.Reward)
            assert np.array_equal(o1.Done, o2.Done) and np.array_equal(o1.Truncated, o2.Truncated)
        assert np.array_equal(env.GetState(), twin.GetState()) and env.Tick == twin.Tick
        before_eps, before_stats = mem.Episodes(), mem.Stats()
        d_a = _dev(rng.integers(0, 2, n).astype(np.int32))
        assert lib.gymnet_vecenv_memory_push_device(h, C.c_void_p(d_a.data_ptr()), None) == inv      # no step since the last push
        env.StepDevice(d_a); env.StepDevice(d_a)
        assert lib.gymnet_vecenv_memory_push_device(h, C.c_void_p(d_a.data_ptr()), None) == inv      # a skipped push
        mem.Reset()
        ring = _dev(np.zeros((3, n), np.int32))
        env.RolloutDevice(ring, 3, n, 3)
        assert lib.gymnet_vecenv_memory_push_device(h, C.c_void_p(ring.data_ptr()), None) == inv     # a multi-step rollout
        mem.Reset()
        env.ResetDevice()
        assert lib.gymnet_vecenv_memory_push_device(h, C.c_void_p(d_a.data_ptr()), None) == inv      # a reset without a memory reset
        assert lib.gymnet_vecenv_memory_push_device(h, None, None) == inv
        assert lib.gymnet_vecenv_memory_config(h, -1, 0, 4) == inv
        assert lib.gymnet_vecenv_memory_config(h, 8, 0, 0) == inv
        assert lib.gymnet_vecenv_memory_dataset_device(h, 7, 200, 150, 200, 150, 40, 20, None, None, None, None, 1) == inv
        assert lib.gymnet_vecenv_memory_dataset_device(h, 0, 0, 0, 0, 0, 0, 0, None, None, None, None, -1) == inv
        ep = [np.empty(4, np.float32), np.empty(4, np.int32), np.empty(4, np.uint64), np.empty(4, np.int32)]
        for e in ep:
            e.view(np.uint8).fill(0x5A)
        assert lib.gymnet_vecenv_memory_episodes(h, *(e.ctypes.data_as(C.c_void_p) for e in ep), -1, None) == inv
        assert all((e.view(np.uint8) == 0x5A).all() for e in ep)
        after = mem.Episodes()
        assert all(np.array_equal(x, y) for x, y in zip(before_eps, after)) and mem.Stats() == before_stats
        x = torch.full((4, 16), 7.0, device="cuda")
        assert lib.gymnet_vecenv_memory_dataset_device(h, 0, 0, 0, 0, 0, 0, 0, C.c_void_p(x.data_ptr()), None, None, None, 0) == 0
        env.Sync()
        assert (x == 7.0).all()


def test_pixel_formats_need_cartpole_and_a_memory(gpu_pkg):
    with gpu_pkg.VectorEnv("Acrobot-v1", 64, seed=SEED, auto_reset=True) as env:
        env.Reset()
        lib, h = env._lib, env._h
        assert lib.gymnet_vecenv_memory_push_device(h, None, None) == gpu_pkg._capi.ERR_INVALID_ARG                  # none configured
        assert lib.gymnet_vecenv_memory_config(h, 4, 0, 2) == gpu_pkg._capi.ERR_INVALID_ARG                          # no max_episode_steps
        mem = env.EpisodeMemory(capacity=4, max_length=50, history=2)
        assert lib.gymnet_vecenv_memory_dataset_device(h, 2, 200, 150, 200, 150, 40, 20, None, None, None, None, 1) == gpu_pkg._capi.ERR_UNSUPPORTED
        mem.Close()
        assert lib.gymnet_vecenv_memory_stats(h, None, None, None, None) == gpu_pkg._capi.ERR_INVALID_ARG


# ---- edges: long episodes, 64-bit ticks, a truncated dataset, the caller's done bytes --------------------------------------------------------

def _balancing(env, rng, t, obs):
    """push towards the side the pole falls to (theta + theta_dot + 0.1 x + 0.3 x_dot > 0), replaced by a uniform draw with probability 0.6:
    episode lengths spread from a dozen steps to the time limit of 200, most of them above 64"""
    x, xd, th, thd = (obs[:, k].astype(np.float64) for k in range(4))
    rule = (th + thd + 0.1 * x + 0.3 * xd > 0).astype(np.int32)
    n = len(rule)
    return np.where(rng.random(n) < 0.6, rng.integers(0, 2, n), rule).astype(np.int32)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_long_episodes_wrap_the_ring_and_take_more_than_one_trip_of_the_copy(gpu_pkg, dtype):
    """max_episode_steps 200: a ring of 201 slots that 420 pushes wrap twice, winners of more than 64 and more than 128 rows (the merge
    copies 64 rows per trip), and short ones beside them; the kept set after every push, the params dataset at the end."""
    short = []
    m, rows = _loop(gpu_pkg, "CartPole-v1", 512, 64, 420, every_push=True, dtype=dtype, max_steps=200, policy=_balancing,
                    after_push=lambda m, t: short.append(min((e["len"] for e in m.pool), default=10 ** 9)))
    assert max(e["len"] for e in m.pool) > 128                                # the final pool holds an episode longer than 128 rows
    assert min(short) <= 64                                                   # and an episode of 64 rows or fewer was admitted
    assert rows > 0


def test_pendulum_episodes_of_exactly_150_rows_arrive_256_at_a_time(gpu_pkg):
    m, rows = _loop(gpu_pkg, "Pendulum-v1", 256, 20, 320, every_push=True, max_steps=150)
    assert m.ended == 512 and len(m.pool) == 20 and all(e["len"] == 150 for e in m.pool) and rows == 20 * 100


def test_pixel_dataset_of_long_episodes_equals_the_pixel_stack_at_action_time(gpu_pkg):
    n, capacity, depth, steps = 512, 4, 2, 420
    crop, size = (200, 150, 200, 150), (40, 20)
    rng = np.random.default_rng(n + capacity)
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=200) as env:
        obs0 = env.Reset()
        stack = env.PixelStack(depth=depth, size=size, crop=crop, format="gray8")
        mem = env.EpisodeMemory(capacity=capacity, max_length=0, history=depth)
        m = model.EpisodeMemoryModel(obs0, capacity, 200, depth)
        seen = []                                                         # history index t -> the stacks when step t's action was chosen
        obs = obs0
        for t in range(steps):
            env.Sync()
            seen.append(stack.Tensor.cpu().numpy())
            a = _balancing(env, rng, t, obs)
            d_a = _dev(a)
            env.StepDevice(d_a)
            stack.Push()
            mem.Push(d_a)
            env.Sync()
            obs = env.GetState().T.copy()
            m.push(a, env.GetArray("reward"), env.GetArray("done"), obs, env.Tick)
        _check_kept(mem, m)
        assert max(e["len"] for e in m.pool) > 64                             # pool rows beyond the 64th are read
        rows = m.dataset_rows()
        gray = np.stack([seen[e["start"] + p][e["lane"]] for e, p, _ in rows])
        x, a, oh = mem.BuildDataset("gray8", size=size, crop=crop, min_episodes=capacity)
        assert np.array_equal(x.cpu().numpy(), stack_model.process(gray, 2))


def test_end_ticks_across_2_to_the_32(gpu_pkg):
    """the radix select's tick digits: the kept set after every push while the end ticks cross 2^32, and Episodes() returns them whole"""
    sc = model.TICKS_ACROSS_2_32
    both = []
    m, rows = _loop(gpu_pkg, "CartPole-v1", sc["n"], sc["capacity"], sc["pushes"], every_push=True, max_steps=sc["max_steps"],
                    start_tick=sc["start_tick"], after_push=lambda m, t: both.append(model.ticks_on_both_sides(m)))
    assert any(both)                                                          # at some push the pool held end ticks on both sides of 2^32
    assert all(e["tick"] > sc["start_tick"] for e in m.pool) and max(e["tick"] for e in m.pool) > 2 ** 32


def test_a_dataset_call_with_fewer_rows_than_the_dataset_stops_there(gpu_pkg):
    import torch

    def truncated(env, mem, m):
        x, a, oh, r = m.dataset_params(env.ActionSpace.N)
        rows, keep = len(x), len(x) - 5
        assert keep > 0
        out = [torch.full(shape, 0x5A, dtype=torch.uint8, device="cuda") for shape in ((rows, x.shape[1] * 4), (rows, 4), (rows, 2 * 4), (rows, 4))]
        torch.cuda.synchronize()
        assert env._lib.gymnet_vecenv_memory_dataset_device(env._h, 0, 0, 0, 0, 0, 0, 0, *(C.c_void_p(o.data_ptr()) for o in out), keep) == 0
        env.Sync()
        got = [o.cpu().numpy() for o in out]
        for g, w in zip(got, (x, a.astype(np.int32), oh, r)):
            w = np.ascontiguousarray(w).reshape(rows, -1)
            assert np.array_equal(g[:keep], w[:keep].view(np.uint8)) and (g[keep:] == 0x5A).all()
    _loop(gpu_pkg, "CartPole-v1", 1024, 64, 100, every_push=False, then=truncated)


def test_pushes_with_the_callers_done_bytes(gpu_pkg):
    """done = the handle's OR a host-chosen 5 % mask, passed to Push and to the model: episodes end where the caller says"""
    m, rows = _loop(gpu_pkg, "CartPole-v1", 1024, 100, 120, every_push=True, own_done=0.05)
    assert m.ended > 1024 and rows > 0
