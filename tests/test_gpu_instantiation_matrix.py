"""Every step, rollout and resident kernel instantiation against the oracle, bit for bit (tests/_instantiation_matrix.py is the table;
tests/test_instantiation_coverage.py pins it to the compiled set).

Step recipes: the launcher must resolve to the recipe's instantiation (KernelName(), GetLaunchPolicy()); start states force the edges
— a quarter of the lanes one step from termination, one whole wave in which every lane finishes (the partial last wave) and one in
which none does, Pendulum angles near multiples of 2 pi, actions beyond the bounds and -0.0 — and 18 steps are replayed on the CPU:
the oracle's kernel-semantics step, the fused reset drawn at (seed or the lane's own key, lane_offset + lane, tick), the bookkeeping
in NumPy.  State, observation, reward, done byte, steps_beyond_done, the done list and the dense episode views must be equal.
Rollout recipes: the preconditions of the intended width are asserted from the buffers (so the library's silent narrower fallback
cannot be taken), then ONE launch of T steps is replayed the same way, with the actions from the ring, the oracle's
ActionSpace.Sample() / Box sample or the epsilon-greedy composer; every recorded step, the final state, the dense views and the
sorted (t, lane, return, length) records must be equal.  Resident recipes: the same replay through the mailbox path."""
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _instantiation_matrix as M  # noqa: E402
from _handle_replay import KEYS, SEED, Replay, _lane_seeds  # noqa: E402,F401  (the replay: the handle's semantics on the CPU)

pytestmark = pytest.mark.gpu
ASEED = 0xAC710
STEPS, T_ROLLOUT, RING, EPS = 18, 16, 5, 0.4

RECIPES = M.recipes()


def _eq(a, b):
    """Exact equality; NaN equals NaN (the recorded CartPole edge states include non-finite ones)."""
    return np.array_equal(a, b, equal_nan=True)


def _by(fam):
    return [pytest.param(r, id=r["name"]) for r in RECIPES if r["family"] == fam]


# ---- start states and actions -----------------------------------------------------------------------------------------------
def _waves(r):
    """(lanes of the wave where every lane finishes, lanes of a wave where none does): the last (partial) wave and the second wave."""
    n, lanes = r["n"], 64 * r["vec"] * r.get("items", 1)
    last = np.arange((n - 1) // lanes * lanes, n)
    if len(last) < lanes // 2 and n > 3 * lanes:          # a sliver: finish the whole wave before it too
        last = np.arange(max(0, last[0] - lanes), n)
    none = np.arange(lanes, min(2 * lanes, last[0]))
    return last, none


def _start(r, golden, rng):
    """Float32 start state [S, n], the edge lanes' step-0 actions (or None), and the lanes that must finish at step 0 / must not."""
    env, n = r["env"], r["n"]
    fin, keep = _waves(r)
    edge = rng.random(n) < 0.25
    edge[fin] = True
    edge[keep] = False
    a0 = None
    if env in ("CartPole", "CartPole64"):
        s = rng.uniform(-0.04, 0.04, (4, n))
        g = golden("cartpole_edges")
        pick = rng.integers(0, g["state"].shape[1], n)
        s[:, edge] = g["state"][:, pick[edge]]                                    # the recorded edge states and their actions
        a0 = np.where(edge, g["action"][pick], -1)
        side = np.where(rng.random(len(fin)) < 0.5, -1.0, 1.0)                    # certain terminals: the pole past its threshold next step
        s[:, fin] = np.stack([rng.uniform(-1, 1, len(fin)), rng.uniform(-1, 1, len(fin)), 0.2 * side, 3.0 * side])
        a0[fin] = -1
        must = fin
    elif env == "MountainCar":
        s = np.stack([rng.uniform(-0.6, -0.4, n), rng.uniform(-0.01, 0.01, n)])
        s[:, edge] = np.stack([rng.uniform(0.45, 0.5, edge.sum()), rng.uniform(0.0, 0.07, edge.sum())])
        s[:, fin] = np.stack([rng.uniform(0.47, 0.5, len(fin)), rng.uniform(0.04, 0.07, len(fin))])      # past the flag whatever the push
        must = fin
    elif env == "Acrobot":
        s = rng.uniform(-0.1, 0.1, (4, n))
        s[:, edge] = np.stack([np.pi - rng.uniform(0, 0.1, edge.sum()), rng.uniform(-0.1, 0.1, edge.sum()),
                               rng.uniform(-4, 4, edge.sum()), rng.uniform(-9, 9, edge.sum())])
        s[:, fin] = np.stack([np.pi - rng.uniform(0, 0.02, len(fin)), rng.uniform(-0.02, 0.02, len(fin)),
                              rng.uniform(-0.3, 0.3, len(fin)), rng.uniform(-0.3, 0.3, len(fin))])          # upright: terminal next step
        must = fin
    else:                                                                          # Pendulum: no termination, only the time limit
        s = np.stack([rng.uniform(-np.pi, np.pi, n), rng.uniform(-8, 8, n)])
        k = rng.integers(-3000, 3000, n)                                           # |theta| < 65536: no libm fallback
        s[0, edge] = (2 * np.pi * k[edge] + rng.choice([0.0, 1e-6, -1e-6, 3e-4], edge.sum())).astype(np.float32)
        s[:, rng.random(n) < 0.02] = -0.0
        must = fin if (r["episode_stats"] and r["max_episode_steps"]) else np.arange(0)
    return s.astype(np.float32), a0, must, keep


def _actions(r, rng, n):
    if r["env"] == "Pendulum":
        a = rng.uniform(-2.5, 2.5, n).astype(np.float32)
        a[rng.random(n) < 0.05] = -0.0
        far = rng.random(n) < 0.05                                                 # beyond the bounds: clamped
        a[far] = rng.choice(np.float32([-50.0, 3.5, -2.0001, 2.0001]), far.sum())
        return a
    return rng.integers(0, M.ENVS[r["env"]]["nvals"], n).astype(np.int32)


def _open(gpu_pkg, r, **more):
    kw = dict(seed=SEED, auto_reset=r["auto_reset"], dtype=np.float64 if r["f64"] else np.float32, lane_offset=r["lane_offset"],
              done_list=r["done_list"], episode_stats=r["episode_stats"], final_obs=r["final_obs"], max_episode_steps=r["max_episode_steps"],
              double_buffer=r["double_buffer"], resident=r["resident"])
    kw.update(more)
    return gpu_pkg.VectorEnv(r["gym"], r["n"], **kw)


def _prepare(env, r, golden, rng):
    """Seeds, reset, forced start state and running statistics; returns the Replay and the step-0 edge actions."""
    if r["lane_seeds"]:
        env.Seed(_lane_seeds(r["n"]).astype(np.int64))
    if r["resident"]:
        env.Reset()
    else:
        env.ResetDevice()
    s0, a0, must, keep = _start(r, golden, rng)
    env.SetState(s0)
    ln0 = ret0 = None
    if r["episode_stats"]:
        ln0 = rng.integers(0, max(r["max_episode_steps"], 6), r["n"]).astype(np.int32)
        if r["max_episode_steps"]:
            ln0[must] = r["max_episode_steps"] - 1
            ln0[keep] = 0
        ret0 = rng.uniform(-3, 3, r["n"]).astype(np.float32)
        env.SetArray("episode_length", ln0)
        env.SetArray("episode_return", ret0)
    sbd0 = env.GetStepsBeyondDone() if (not r["auto_reset"] and r["env"].startswith("CartPole")) else None
    return Replay(env_oracle(), r, env.GetState(), sbd0, ln0, ret0), s0, a0, must, keep


_ORACLE = []


def env_oracle():
    return _ORACLE[0]


@pytest.fixture(autouse=True)
def _oracle_ref(oracle):
    if not _ORACLE:
        _ORACLE.append(oracle)


def _check_dense(env, rp):
    r = rp.r
    if r["episode_stats"]:
        assert _eq(env.GetArray("episode_length"), rp.ln) and _eq(env.GetArray("episode_return"), rp.ret)
        if not r["resident"]:
            assert _eq(env.GetArray("finished_length"), rp.fin_len)
            assert _eq(env.GetArray("finished_return"), rp.fin_ret)
    if r["final_obs"]:
        assert _eq(env.GetArray("final_obs"), rp.final)


# ---- step recipes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", _by("step_kernel") + _by("step_kernel_pipe") + _by("step_kernel_pipe2") + _by("step_kernel_lds"))
def test_step_instantiation_equals_the_oracle(gpu_pkg, golden, r):
    rng = np.random.default_rng(zlib.crc32(r["name"].encode()))
    with _open(gpu_pkg, r, launch_policy=r["launch"]) as env:
        rp, s0, a0, must, keep = _prepare(env, r, golden, rng)                 # (per-lane seeds select the bookkeeping variant)
        assert env.KernelName() == r["name"]
        pol = env.GetLaunchPolicy()
        assert all(pol[k] == v for k, v in r["launch"].items()), (pol, r["launch"])
        assert _eq(env.GetState(), s0.astype(rp.s.dtype))
        for t in range(STEPS):
            a = _actions(r, rng, r["n"])
            if t == 0 and a0 is not None:
                a = np.where(a0 >= 0, a0, a).astype(np.int32)
            tick = env.Tick
            out = env.Step(a)
            obs, rw, db, fin = rp.step(a, tick)
            if t == 0:
                assert fin[must].all() and not fin[keep].any()                         # the forced edges took place
            assert _eq(env.GetState(), rp.s), (t, _first_diff(env.GetState(), rp.s))
            assert _eq(out.Observation, obs.T), (t, _first_diff(out.Observation.T, obs))
            assert _eq(out.Reward, rw) and _eq(env.GetArray("done"), db), t
            if rp.sbd is not None:
                assert _eq(env.GetStepsBeyondDone(), rp.sbd), t
            if r["done_list"]:
                assert _eq(np.sort(env.DoneLanes()), np.nonzero(fin)[0]), t
                rec = env.DoneRecords()
                order = np.argsort(rec["lanes"])
                if r["episode_stats"]:
                    assert _eq(rec["return"][order], rp.fin_ret[fin]) and _eq(rec["length"][order], rp.fin_len[fin]), t
                if r["final_obs"]:
                    assert _eq(rec["final_obs"][order], rp.final[:, fin].T), t
        assert env.KernelName() == r["name"]
        _check_dense(env, rp)


def _first_diff(a, b):
    d = np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))
    return None if len(d) == 0 else (tuple(int(x) for x in d[0]), a[tuple(d[0])], b[tuple(d[0])])


# ---- rollout recipes -------------------------------------------------------------------------------------------------------
def _episode_buffers(torch, cap, no_overflow):
    ep = dict(step=torch.full((cap,), -1, dtype=torch.int32, device="cuda"), lane=torch.full((cap,), -1, dtype=torch.int32, device="cuda"),
              ret=torch.zeros(cap, dtype=torch.float32, device="cuda"), length=torch.zeros(cap, dtype=torch.int32, device="cuda"),
              capacity=cap, count=torch.zeros(2, dtype=torch.uint32, device="cuda"))
    if no_overflow:
        ep["no_overflow"] = True
    return ep


@pytest.mark.parametrize("r", _by("rollout_kernel"))
def test_rollout_instantiation_equals_the_oracle(gpu_pkg, golden, r):
    import torch
    rng = np.random.default_rng(zlib.crc32(r["name"].encode()))
    n, T, v, src = r["n"], T_ROLLOUT, r["vec"], r["actions"]
    box = M.ENVS[r["env"]]["box"]
    adt = torch.float32 if box else torch.int32
    rdt = torch.float64 if r["f64"] else torch.float32
    with _open(gpu_pkg, r, launch_policy=r["launch"]) as env:
        rp, s0, a0, must, keep = _prepare(env, r, golden, rng)
        O = env.ObsDim
        ring = torch.from_numpy(np.stack([_actions(r, rng, n) for _ in range(RING)])).cuda() if src != "sample" else None
        rec_o = torch.zeros((T, O, n), dtype=rdt, device="cuda")
        rec_r = torch.zeros((T, n), dtype=torch.float32, device="cuda")
        rec_d = torch.zeros((T, n), dtype=torch.uint8, device="cuda")
        rec_a = torch.zeros((T, n), dtype=adt, device="cuda") if r["rec_actions"] else None
        # no_overflow: the capacity keeps every shard's own segment (2 * ceil(capacity / 256) + 64 records) from filling — a wave
        # whose lanes all finish at every step appends 64 * v * T records
        cap = max(n * T, 128 * 64 * v * T) if r["records"] == "no_overflow" else n * T
        assert r["records"] != "no_overflow" or 2 * (-(-cap // 256)) + 64 >= 64 * v * T
        ep = _episode_buffers(torch, cap, r["records"] == "no_overflow") if r["records"] != "none" else None
        bufs = [x for x in (ring, rec_o, rec_r, rec_d, rec_a) if x is not None]
        # the preconditions of the intended width: every stream 16-byte aligned, n and the action stride whole lane groups
        assert all(b.data_ptr() % 16 == 0 for b in bufs)
        assert v == 1 or (n % v == 0 and (ring is None or ring.stride(0) % v == 0))
        assert (ring.stride(0) if ring is not None else None) == r["action_stride"]
        name, got_v = M.rollout_instantiation(r["env"], env.GetLaunchPolicy()["vec"], n, r["auto_reset"], r["name"].split(",")[3] == "true",
                                              src, ep is not None, r["records"] == "no_overflow", env.GetLaunchPolicy()["reset_form"],
                                              action_stride=r["action_stride"])
        assert name == r["name"] and got_v == v
        tick0 = env.Tick
        torch.cuda.synchronize()
        env.RolloutFusedDevice(ring, T, n if ring is not None else 0, RING, rec_obs=rec_o, rec_reward=rec_r, rec_done=rec_d, rec_actions=rec_a,
                               actions=src, action_seed=ASEED, action_tick0=1000 + r["lane_offset"] % 7, epsilon=EPS, episodes=ep)
        env.Sync()
        assert env.Tick == tick0 + T
        got_o, got_r, got_d = rec_o.cpu().numpy(), rec_r.cpu().numpy(), rec_d.cpu().numpy()
        got_a = rec_a.cpu().numpy() if rec_a is not None else None
        pol = ring.cpu().numpy() if ring is not None else None
        want, want_ret = [], []
        lo, atick0, nv = r["lane_offset"], 1000 + r["lane_offset"] % 7, M.ENVS[r["env"]]["nvals"]
        for t in range(T):
            if src == "ring":
                a = pol[t % RING]
            elif src == "sample":
                a = (M_box_sample(lo, atick0 + t, n) if box else env_oracle().discrete_sample(ASEED, lo, atick0 + t, nv, 0, n))
            else:
                a = env_oracle().compose_discrete(ASEED, lo, atick0 + t, nv, EPS, pol[t % RING])
            if got_a is not None:
                assert _eq(got_a[t], a), t
            obs, rw, db, fin = rp.step(a, tick0 + t)
            assert _eq(got_o[t], obs), (t, _first_diff(got_o[t], obs))
            assert _eq(got_r[t], rw) and _eq(got_d[t], db), t
            lanes = np.nonzero(fin)[0]
            want.append(np.stack([np.full(len(lanes), t), lanes, rp.fin_len[fin] if rp.stats else np.zeros(len(lanes), np.int32)], axis=1))
            want_ret.append(rp.fin_ret[fin].copy())
        assert _eq(env.GetState(), rp.s), _first_diff(env.GetState(), rp.s)
        if rp.sbd is not None:
            assert _eq(env.GetStepsBeyondDone(), rp.sbd)
        _check_dense(env, rp)
        if r["done_list"]:
            assert _eq(np.sort(env.DoneLanes()), lanes)                    # the done list describes the rollout's last step
        if ep is not None:
            c = ep["count"].cpu().numpy().astype(np.int64)
            k = int(c[0])
            rec = np.stack([ep["step"].cpu().numpy()[:k], ep["lane"].cpu().numpy()[:k], ep["length"].cpu().numpy()[:k]], axis=1)
            got_ret = ep["ret"].cpu().numpy()[:k]
            order = np.lexsort((rec[:, 1], rec[:, 0]))
            want = np.concatenate(want)
            assert c[0] == c[1] == len(want) > 0
            assert _eq(rec[order], want) and _eq(got_ret[order], np.concatenate(want_ret))


def M_box_sample(lo, tick, n):
    return env_oracle().box_uniform_sample(ASEED, lo, tick, -2.0, 2.0, n)


# ---- resident recipes ------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("r", _by("resident_kernel"))
def test_resident_instantiation_equals_the_oracle(gpu_pkg, golden, r):
    rng = np.random.default_rng(zlib.crc32(r["name"].encode()))
    with _open(gpu_pkg, r) as env:
        rp, s0, a0, must, keep = _prepare(env, r, golden, rng)
        for t in range(STEPS):
            a = _actions(r, rng, r["n"])
            if t == 0 and a0 is not None:
                a = np.where(a0 >= 0, a0, a).astype(np.int32)
            tick = env.Tick
            out = env.Step(a)
            obs, rw, db, fin = rp.step(a, tick)
            assert _eq(out.Observation, obs.T), (t, _first_diff(out.Observation.T, obs))
            assert _eq(out.Reward, rw) and _eq(out.Done, fin) and _eq(out.Truncated, (db & 2) != 0), t
        assert env.Tick == tick + 1
        assert _eq(env.GetState(), rp.s)
        if rp.sbd is not None:
            assert _eq(env.GetStepsBeyondDone(), rp.sbd)
        _check_dense(env, rp)


# ---- record_flags validation -------------------------------------------------------------------------------------------------
def test_unknown_record_flags_are_refused_without_side_effects(gpu_pkg):
    """gymnet_rollout_spec.record_flags was `reserved` under ABI 5: a bit other than GYMNET_RECORDS_NO_OVERFLOW is an error, and the
    refused call launches nothing — tick, state and record count are unchanged."""
    import ctypes as C
    import torch
    capi = gpu_pkg._capi
    n, T = 2048, 8
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True, episode_stats=True) as env:
        env.ResetDevice()
        ep = _episode_buffers(torch, n * T, False)
        ep["count"].fill_(12345)
        before, tick = env.GetState(), env.Tick
        torch.cuda.synchronize()
        for bad in (2, 0x100, -1, 1 | 4):
            spec = capi.RolloutSpec(struct_size=C.sizeof(capi.RolloutSpec), action_source=capi.ACTIONS_SAMPLE, steps=T, ring=1,
                                    action_seed=ASEED, record_flags=bad, d_ep_step=ep["step"].data_ptr(), d_ep_lane=ep["lane"].data_ptr(),
                                    d_ep_return=ep["ret"].data_ptr(), d_ep_length=ep["length"].data_ptr(), ep_capacity=n * T,
                                    d_ep_count=ep["count"].data_ptr())
            with pytest.raises(ValueError, match="record_flags"):
                capi.check(env._lib.gymnet_vecenv_rollout_fused_ex_device(env._h, C.byref(spec)))
        env.Sync()
        assert env.Tick == tick and _eq(env.GetState(), before)
        assert (ep["count"].cpu().numpy() == 12345).all()
        env.RolloutFusedDevice(None, T, actions="sample", action_seed=ASEED, episodes=ep)           # 0 and NO_OVERFLOW still work
        env.RolloutFusedDevice(None, T, actions="sample", action_seed=ASEED, episodes=dict(ep, no_overflow=True))
        env.Sync()
        assert env.Tick == tick + 2 * T
