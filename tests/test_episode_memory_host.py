"""CPU checks of the episode memory (gymnet_vecenv_memory_*): the NumPy model's top-K-per-push form equals the reference's sequential
EndEpisode rule applied one episode at a time in (tick, lane) order, over random and tie-heavy streams; the model's bookkeeping and
dataset on a hand-worked sequence; and the library exports the seven calls, the header, ctypes and Native.cs declare them with the same
arity, every host wrapper reaches them, and calls on a null handle are refused without writing anything."""
import ctypes
import os
import re

import numpy as np
import pytest

import _episode_memory_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"gymnet_vecenv_memory_config": 4, "gymnet_vecenv_memory_reset_device": 3, "gymnet_vecenv_memory_push_device": 3,
         "gymnet_vecenv_memory_stats": 5, "gymnet_vecenv_memory_episodes": 7, "gymnet_vecenv_memory_dataset_size": 2,
         "gymnet_vecenv_memory_dataset_device": 13}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _arity(text, name):
    m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*[;{]" % name, text, flags=re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])


def _stream(rng, pushes, lanes_per_push, ret_values):
    """Per push: the episodes that ended in it (ticks increase with the push, lanes distinct within a push)."""
    out = []
    for t in range(pushes):
        k = int(rng.integers(0, lanes_per_push + 1))
        lanes = rng.choice(1000, size=k, replace=False)
        out.append([{"ret": np.float32(ret_values(rng)), "len": 1, "tick": 10 + t, "lane": int(l)} for l in lanes])
    return out


@pytest.mark.parametrize("capacity", [1, 3, 10, 100])
@pytest.mark.parametrize("kind", ["random", "ties", "negative"])
def test_top_k_per_push_equals_the_sequential_rule(capacity, kind):
    rng = np.random.default_rng(capacity * 7 + len(kind))
    values = {"random": lambda r: r.normal(50.0, 20.0),
              "ties": lambda r: float(r.integers(8, 14)),                 # CartPole-like integer returns: ties are the common case
              "negative": lambda r: -float(r.integers(0, 5)) * 0.5}[kind]
    pool_seq, pool_push = [], []
    for ended in _stream(rng, 200, 12, values):
        for e in sorted(ended, key=lambda e: (e["tick"], e["lane"])):     # the reference's order: oldest first
            pool_seq = model.end_episode_sequential(pool_seq, e, capacity)
        pool_push = model.top_k_per_push(pool_push, ended, capacity)
        assert sorted(map(model.key, pool_seq)) == sorted(map(model.key, pool_push))
    assert len(pool_push) == capacity


def test_newer_wins_ties():
    old = {"ret": np.float32(10), "len": 3, "tick": 5, "lane": 9}
    new = {"ret": np.float32(10), "len": 4, "tick": 6, "lane": 0}
    same_tick = {"ret": np.float32(10), "len": 2, "tick": 6, "lane": 1}
    assert model.top_k_per_push([old], [new], 1) == [new]
    assert model.top_k_per_push([old], [new, same_tick], 1) == [same_tick]
    assert model.end_episode_sequential([old], new, 1) == [new]
    assert model.end_episode_sequential([new], {"ret": np.float32(9.5), "len": 1, "tick": 7, "lane": 3}, 1) == [new]


def test_model_hand_worked_sequence():
    """Two lanes, history 2, capacity 1, auto-reset: lane 0 ends after 3 steps (return 3), lane 1 after 4 (return 4, kept)."""
    obs0 = np.array([[0.0, 0.5], [10.0, 10.5]], np.float32)
    m = model.EpisodeMemoryModel(obs0, capacity=1, max_length=10, history=2)
    for t in range(4):
        obs = obs0 + (t + 1)
        done = np.array([t == 2, t == 3], np.uint8)
        if t == 3:
            obs[0] = [100.0, 100.5]
        m.push(np.array([t % 2, 1 - t % 2], np.int32), np.ones(2, np.float32), done, obs, end_tick=t + 1)
    ret, ln, tick, lane = m.kept()
    assert ret.tolist() == [4.0] and ln.tolist() == [4] and tick.tolist() == [4] and lane.tolist() == [1]
    assert (m.ended, m.admitted, m.too_long) == (2, 2, 0)
    x, a, oh, r = m.dataset_params(action_n=2)
    # floor(4 * 2 / 3) = 2 rows: (o_0, o_0) and (o_0, o_1), the oldest first
    assert x.tolist() == [[10.0, 10.5, 10.0, 10.5], [10.0, 10.5, 11.0, 11.5]]
    assert a.tolist() == [1, 0] and oh.tolist() == [[0, 1], [1, 0]] and r.tolist() == [1.0, 1.0]
    # lane 0's second episode opened from its post-step observation at the push that ended the first
    assert m.start[0] == 3 and np.array_equal(m.obs[3][0], obs0[0] + 3)


def test_model_too_long_closed_lanes_and_reset():
    obs0 = np.zeros((3, 1), np.float32)
    m = model.EpisodeMemoryModel(obs0, capacity=4, max_length=2, history=1, autoreset=False)
    m.push(np.zeros(3, np.int32), np.ones(3, np.float32), [1, 0, 0], obs0 + 1, 1)
    m.push(np.zeros(3, np.int32), np.ones(3, np.float32), [1, 0, 0], obs0 + 2, 2)     # lane 0 is closed: nothing recorded
    m.push(np.zeros(3, np.int32), np.ones(3, np.float32), [0, 1, 0], obs0 + 3, 3)     # lane 1: 3 steps > max_length 2
    assert (m.ended, m.too_long) == (2, 1) and m.kept()[3].tolist() == [0]
    m.reset(obs0 + 7, mask=[1, 1, 0])
    m.push(np.zeros(3, np.int32), np.ones(3, np.float32), [1, 0, 1], obs0 + 8, 5)
    ret, ln, tick, lane = m.kept()
    assert ret.tolist() == [1.0, 1.0] and ln.tolist() == [1, 1] and tick.tolist() == [5, 1] and lane.tolist() == [0, 0]
    assert (m.ended, m.too_long) == (4, 2)                                            # lane 2: 4 steps
    m.reset(obs0, clear=True)
    assert m.kept()[0].size == 0 and m.ended == 0


def test_the_2_to_the_32_scenario_puts_end_ticks_on_both_sides_of_the_boundary():
    """model.TICKS_ACROSS_2_32, the GPU test's scenario, with the NumPy oracle standing in for the device: float32 CartPole steps, the
    engine's reset draws at the step's tick, the same policy and time limit.  At some push the pool holds end ticks below and above 2^32,
    and the uint64 ticks survive the model's key order (a tick truncated to 32 bits would rank the newer episodes below the older)."""
    from oracle import numpy_ref as ref
    sc = model.TICKS_ACROSS_2_32
    n, seed = sc["n"], 0x5EED
    lanes = np.arange(n)
    rng = np.random.default_rng(n + sc["capacity"])
    s = ref.cartpole_reset(seed, lanes, 0)
    m = model.EpisodeMemoryModel(s.T, sc["capacity"], sc["max_steps"], 4)
    length = np.zeros(n, np.int64)
    tick = sc["start_tick"]
    both = []
    for t in range(sc["pushes"]):
        a = model.mixed_policy(n, rng, t)
        s, r, d, _ = ref.cartpole_step(s, a, np.full(n, -1, np.int32), dtype=np.float32)
        length += 1
        done = d | (length >= sc["max_steps"])
        s[:, done] = ref.cartpole_reset(seed, lanes, tick)[:, done]           # the fused reset draws at the tick the step started from
        length[done] = 0
        tick += 1
        m.push(a, r, done, s.T, tick)
        both.append(model.ticks_on_both_sides(m))
    assert any(both) and both.index(True) == 2 ** 32 - sc["start_tick"] - 1   # push 39: the first whose end tick is 2^32
    kept_ticks = m.kept()[2]
    assert kept_ticks.dtype == np.uint64 and int(kept_ticks.max()) > 2 ** 32 and len(m.pool) == sc["capacity"]
    newest = max(m.pool, key=model.key)
    assert all(model.key(e) <= model.key(newest) for e in m.pool) and newest["tick"] >= 2 ** 32


def test_library_and_bindings_declare_the_memory_calls(gymnet):
    lib = ctypes.CDLL(gymnet.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", _read("include", "gymnet_amd.h"), flags=re.S)
    native = _read("gym.net_amd", "csharp", "Native.cs")
    for name, n in CALLS.items():
        assert hasattr(lib, name), name
        assert _arity(hdr, name) == n, name
        assert name in gymnet._capi.PROTOTYPES and len(gymnet._capi.PROTOTYPES[name][1]) == n, name
        assert re.search(r"\[DllImport\(Lib\)\] public static extern int %s\(" % name, native), name
        assert _arity(native, name) == n, name
    assert "enum { GYMNET_MEMORY_PARAMS = 0 };" in hdr
    assert gymnet._capi.MEMORY_PARAMS == 0
    assert "MemoryParams = 0" in native


def test_host_wrappers_reach_every_call():
    cs = re.sub(r"//.*", "", _read("gym.net_amd", "csharp", "VectorEnv.cs"))
    hpp = _read("include", "gymnet_amd.hpp")
    py = _read("gym.net_amd", "vector_env.py")
    for name in CALLS:
        assert "Native.%s(" % name in cs, name
        assert "%s(" % name in hpp, name
        assert "%s(" % name in py, name
    for m in ("public void ConfigureEpisodeMemory(", "public void PushEpisodeMemory(", "public void ResetEpisodeMemory(",
              "ReadMemoryEpisodes(", "BuildMemoryDataset("):
        assert m in cs, m
    for m in ("void ConfigureEpisodeMemory(", "void PushEpisodeMemory(", "void ResetEpisodeMemory(", "ReadMemoryEpisodes(",
              "BuildMemoryDataset("):
        assert m in hpp, m


def test_python_api_has_the_memory_members(gymnet):
    assert callable(gymnet.VectorEnv.EpisodeMemory)
    for m in ("Push", "Step", "Reset", "Stats", "Episodes", "BuildDataset", "DatasetSize", "Close"):
        assert callable(getattr(gymnet.EpisodeMemory, m)), m


def test_calls_on_a_null_handle_are_refused(gymnet):
    lib = gymnet.load_library()
    inv = gymnet._capi.ERR_INVALID_ARG
    buf = np.full(64, 0x5A, np.uint8)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    i64 = [ctypes.c_int64(-7) for _ in range(4)]
    assert lib.gymnet_vecenv_memory_config(None, 100, 0, 4) == inv
    assert lib.gymnet_vecenv_memory_reset_device(None, None, 0) == inv
    assert lib.gymnet_vecenv_memory_push_device(None, p, None) == inv
    assert lib.gymnet_vecenv_memory_stats(None, *(ctypes.byref(v) for v in i64)) == inv
    assert lib.gymnet_vecenv_memory_episodes(None, p, p, p, p, 4, ctypes.byref(i64[0])) == inv
    assert lib.gymnet_vecenv_memory_dataset_size(None, ctypes.byref(i64[1])) == inv
    assert lib.gymnet_vecenv_memory_dataset_device(None, 0, 200, 150, 200, 150, 40, 20, p, p, p, p, 4) == inv
    assert (buf == 0x5A).all() and all(v.value == -7 for v in i64)
