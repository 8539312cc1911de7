"""CPU checks of the episode memory's rollout ingest (gymnet_vecenv_memory_config_rollout / _push_rollout_device): the library exports the
two calls; the header, ctypes, Native.cs, the C++ mirror and vector_env.py declare them with the same arity; a null handle is refused;
the Python wrappers refuse bad counts before any native call; and, with tests/_episode_memory_model.py, the argument the chunked merge
rests on: filtering each push's ended episodes with a threshold that is frozen for C pushes, instead of the current one, changes neither
the pool after any push nor the number of admitted episodes, because the merge decides what is kept."""
import ctypes
import os
import re

import numpy as np
import pytest

import _episode_memory_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"gymnet_vecenv_memory_config_rollout": 5, "gymnet_vecenv_memory_push_rollout_device": 8}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _arity(text, name):
    m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*[;{]" % name, text, flags=re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])


def test_library_and_bindings_declare_the_two_calls(gymnet):
    lib = ctypes.CDLL(gymnet.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", _read("include", "gymnet_amd.h"), flags=re.S)
    native = _read("gym.net_amd", "csharp", "Native.cs")
    for name, n in CALLS.items():
        assert hasattr(lib, name), name
        assert _arity(hdr, name) == n, name
        assert name in gymnet._capi.PROTOTYPES and len(gymnet._capi.PROTOTYPES[name][1]) == n, name
        assert re.search(r"\[DllImport\(Lib\)\] public static extern int %s\(" % name, native), name
        assert _arity(native, name) == n, name
    assert "#define GYMNET_ABI_VERSION 6" in _read("include", "gymnet_amd.h") or gymnet._capi.load_library().gymnet_abi_version() == 6


def test_host_wrappers_reach_the_two_calls(gymnet):
    cs = re.sub(r"//.*", "", _read("gym.net_amd", "csharp", "VectorEnv.cs"))
    hpp = _read("include", "gymnet_amd.hpp")
    py = _read("gym.net_amd", "vector_env.py")
    for name in CALLS:
        assert "Native.%s(" % name in cs, name
        assert "%s(" % name in hpp, name
        assert "%s(" % name in py, name
    for m in ("public void ConfigureEpisodeMemoryRollout(", "public void PushMemoryRollout("):
        assert m in cs, m
    for m in ("void ConfigureEpisodeMemoryRollout(", "void PushMemoryRollout("):
        assert m in hpp, m
    for m in ("PushRollout", "Rollout"):
        assert callable(getattr(gymnet.EpisodeMemory, m)), m


def test_calls_on_a_null_handle_are_refused(gymnet):
    lib = gymnet.load_library()
    inv = gymnet._capi.ERR_INVALID_ARG
    buf = np.full(64, 0x5A, np.uint8)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.gymnet_vecenv_memory_config_rollout(None, 100, 0, 4, 16) == inv
    assert lib.gymnet_vecenv_memory_push_rollout_device(None, 4, p, p, 4, 4, p, p) == inv
    assert (buf == 0x5A).all()


class _NoNativeCalls:
    """stands in for the library: any call through it fails the test"""
    def __getattr__(self, name):
        raise AssertionError(f"native call {name} reached")


def _memory_without_a_library(gymnet, n=8):
    env = gymnet.VectorEnv.__new__(gymnet.VectorEnv)
    env._lib, env._h, env._owns_handle = _NoNativeCalls(), ctypes.c_void_p(1), False
    env.NumberOfEnvironments, env.Device = n, None
    mem = gymnet.EpisodeMemory.__new__(gymnet.EpisodeMemory)
    mem._env, mem._lib, mem._h, mem._rec = env, env._lib, env._h, None
    return env, mem


@pytest.mark.parametrize("bad", [-1, 65, True, 2.0, "4", None])
def test_a_bad_rollout_chunk_is_refused_before_any_native_call(gymnet, bad):
    env, _ = _memory_without_a_library(gymnet)
    with pytest.raises(ValueError, match="rollout_chunk"):
        gymnet.EpisodeMemory(env, 5, 10, 2, rollout_chunk=bad)


@pytest.mark.parametrize("kw,word", [(dict(steps=0), "steps"), (dict(steps=-2), "steps"), (dict(steps=True), "steps"), (dict(steps=1.5), "steps"),
                                     (dict(ring=0), "ring"), (dict(ring=False), "ring"), (dict(action_stride=-1), "action_stride"),
                                     (dict(action_stride=0.5), "action_stride")])
def test_bad_ingest_counts_are_refused_before_any_native_call(gymnet, kw, word):
    _, mem = _memory_without_a_library(gymnet)
    args = dict(steps=4, ring=None, action_stride=None)
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        mem.PushRollout(args.pop("steps"), 1, 1, 1, 1, **args)
    with pytest.raises(ValueError, match="steps"):
        mem.Rollout(kw.get("steps", 0))


# ---- the argument the chunked merge rests on ---------------------------------------------------------------------------------------------
def _stream(rng, pushes, lanes_per_push, ret_values):
    out = []
    for t in range(pushes):
        k = int(rng.integers(0, lanes_per_push + 1))
        lanes = rng.choice(1000, size=k, replace=False)
        out.append([{"ret": np.float32(ret_values(rng)), "len": 1, "tick": 10 + t, "lane": int(l)} for l in lanes])
    return out


def _filtered_merges(stream, capacity, freeze):
    """The device's two stages per push: the admission filter (pool not full, or return >= a threshold), then the top-K merge of what
    passed.  The filter's (full, threshold) pair is read every `freeze` pushes — 1: before every push, as the single push does; C: as they
    stood before the pass, as the rollout ingest does.  Returns the pool's keys after every push and the admitted count."""
    pool, admitted, pools = [], 0, []
    full, thr = False, None
    for t, ended in enumerate(stream):
        if t % freeze == 0:
            full = len(pool) == capacity
            thr = min(float(e["ret"]) for e in pool) if pool else None
        cands = [e for e in ended if not full or float(e["ret"]) >= thr]
        before = {id(e) for e in pool}
        pool = model.top_k_per_push(pool, cands, capacity)
        admitted += sum(1 for e in pool if id(e) not in before)
        pools.append(sorted(map(model.key, pool)))
    return pools, admitted


@pytest.mark.parametrize("capacity", [1, 5, 40])
@pytest.mark.parametrize("kind", ["random", "ties", "negative"])
def test_a_stale_filter_threshold_changes_neither_the_pool_nor_admitted(capacity, kind):
    rng = np.random.default_rng(capacity * 11 + len(kind))
    values = {"random": lambda r: r.normal(50.0, 20.0), "ties": lambda r: float(r.integers(8, 14)),
              "negative": lambda r: -float(r.integers(0, 5)) * 0.5}[kind]
    stream = _stream(rng, 160, 9, values)
    # the contract's own statement, with no filter at all: the top K of (kept set + every episode that ended in the push)
    pool, unfiltered, want_admitted = [], [], 0
    for ended in stream:
        before = {id(e) for e in pool}
        pool = model.top_k_per_push(pool, ended, capacity)
        want_admitted += sum(1 for e in pool if id(e) not in before)
        unfiltered.append(sorted(map(model.key, pool)))
    assert len(pool) == capacity and want_admitted > capacity
    for freeze in (1, 3, 16):
        pools, admitted = _filtered_merges(stream, capacity, freeze)
        assert pools == unfiltered, freeze
        assert admitted == want_admitted, freeze
