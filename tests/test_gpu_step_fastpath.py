"""The body a FULL workgroup of CartPole's lean auto-reset step kernels runs addresses its rows from scalar bases, takes the reset's
ballots straight from the done compares and — for a full wave with at most 64 finished slots — resets in a single trip
(csrc/step_kernels.hpp step_body_wg, reset_finished_wave; csrc/lanes.hpp WgLanes).  None of that may change a bit of any result, so the
wide form is run where each piece can go wrong and compared, bit for bit, with two references: the oracle's batched auto-reset step
(the replay of tests/test_gpu_instantiation_matrix.py) and a handle of the scalar form (vec 1, reset form 0: a full workgroup of it
runs the same body with one lane per thread and the per-thread reset loop; its ragged end the guarded per-lane body) fed the same inputs.

  envs       CartPole float32: all three pieces.  MountainCar, Pendulum and float64 CartPole share the kernel template but keep the
             general body and the round-loop reset (has_full_workgroup_body() is false for them); their cases hold that dispatch,
             and the same sizes, counts and offsets, to the same two references
  sizes      1 lane; 256 * 4 lanes — exactly one full workgroup; 256 * 4 * 2 + 3 — two full workgroups and a ragged one; 3 steps
  finished   start states that make exactly 0, 1, 64, 65 and ALL sub-lanes of the first wave finish at step 0 (single trip, its
             boundary at 64 slots, the round loop behind it); the other waves finish about a quarter of theirs
  offsets    lane offsets 0, 1, 2, 3 and 2^32 + 5 (the Philox counter's global lane: wave base on the scalar unit + slot)
  buffers    in place, double buffer, external observation buffers, and external buffers with an odd stride that forces vec = 1
  paths      StepDevice per step, RolloutDevice eager, RolloutDevice replaying a hipGraph
state, observation, reward, done and the device tick are compared."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _instantiation_matrix as M  # noqa: E402
import test_gpu_instantiation_matrix as T  # noqa: E402  (its Replay; only the module object is imported)

SEED, STEPS, RING, BLOCK = T.SEED, 3, 2, 256
SIZES = (1, BLOCK * 4, BLOCK * 4 * 2 + 3)
OFFSETS = (0, 1, 2, 3, (1 << 32) + 5)
BUFFERS = ("in_place", "double_buffer", "external", "external_odd")
PATHS = ("step", "rollout", "graph")
ODIM = {"CartPole": 4, "CartPole64": 4, "MountainCar": 2, "Pendulum": 3}


def _counts(env, n):
    """finished sub-lanes of the first wave at step 0"""
    wave = 64 * M.wide_of(env)
    if env == "Pendulum":
        return (0,)                                   # never terminates
    return tuple(sorted({min(c, n) for c in (0, 1, 64, 65, wave)}))


def _cases():
    out = []
    for env in ("CartPole", "MountainCar", "Pendulum", "CartPole64"):
        for n in SIZES:
            counts = _counts(env, n)
            if env == "CartPole" and n == SIZES[-1]:
                pairs = [(c, lo) for c in counts for lo in OFFSETS]                   # the headline form: every count at every offset
            else:
                pairs = [(counts[k % len(counts)], lo) for k, lo in enumerate(OFFSETS)]
            out += [pytest.param(env, n, c, lo, id=f"{env}-n{n}-fin{c}-lo{lo}") for c, lo in pairs]
    return out


def _terminal(env, rng, k):
    """k states that finish at the next step whatever the action"""
    if env == "MountainCar":
        return np.stack([rng.uniform(0.47, 0.5, k), rng.uniform(0.04, 0.07, k)])
    side = np.where(rng.random(k) < 0.5, -1.0, 1.0)
    return np.stack([rng.uniform(-1, 1, k), rng.uniform(-1, 1, k), 0.2 * side, 3.0 * side])


def _start(env, n, count, rng):
    """[S, n] start state: `count` finishing lanes among the first wave's, about a quarter of the lanes behind it"""
    if env == "Pendulum":
        return np.stack([rng.uniform(-np.pi, np.pi, n), rng.uniform(-8, 8, n)]).astype(np.float32)
    s = np.stack([rng.uniform(-0.6, -0.4, n), rng.uniform(-0.01, 0.01, n)]) if env == "MountainCar" else rng.uniform(-0.04, 0.04, (4, n))
    wave = min(n, 64 * M.wide_of(env))
    fin = np.zeros(n, bool)
    fin[rng.permutation(wave)[:count]] = True
    fin[wave:] = rng.random(n - wave) < 0.25
    s[:, fin] = _terminal(env, rng, int(fin.sum()))
    return s.astype(np.float32)


def _recipe(env, n, lane_offset, vec):
    e = M.ENVS[env]
    return dict(env=env, gym=e["gym"], n=n, f64=e["f64"], vec=vec, items=1, lane_seeds=False, auto_reset=True, episode_stats=False,
                max_episode_steps=0, final_obs=False, lane_offset=lane_offset, done_list=False)


def _run(gpu_pkg, torch, r, policy, name_prefix, buffers, path, s0, ring, stride, replay=None):
    """STEPS steps on one fresh handle; returns (state, observation, reward, done, ticks).  replay: compare every step with the oracle."""
    n, dt = r["n"], (np.float64 if r["f64"] else np.float32)
    kw, keep = {}, []
    if buffers == "double_buffer":
        kw["double_buffer"] = True
    elif buffers.startswith("external"):
        ostride = stride + 1 if buffers == "external_odd" else stride       # odd stride: rows 2..O of the buffer are not 16-byte aligned
        ext = torch.zeros(ODIM[r["env"]] * ostride, dtype=torch.float64 if r["f64"] else torch.float32, device="cuda")
        keep.append(ext)
        kw.update(ext_obs=ext.data_ptr(), ext_obs_stride=ostride)
        torch.cuda.synchronize()                                            # the handle launches on a stream of its own
    with gpu_pkg.VectorEnv(r["gym"], n, seed=SEED, auto_reset=True, dtype=dt, lane_offset=r["lane_offset"], **kw) as env:
        if buffers == "external_odd":
            env.SetLaunchPolicy(graph=1 if path == "graph" else 0)          # the library's own choice: it must fall back to vec 1
            name_prefix = f"step_kernel<{r['env']},1,true,false,"
        else:
            env.SetLaunchPolicy(graph=1 if path == "graph" else 0, **policy)
        name = env.KernelName()
        assert name.startswith(name_prefix), (name, name_prefix)
        env.ResetDevice()
        env.SetState(s0)
        tick0 = env.Tick
        if path == "step":
            for t in range(STEPS):
                env.StepDevice(ring[t % RING])
                if replay is not None:
                    env.Sync()
                    out = env.Read()
                    obs, rw, db, fin = replay.step(ring[t % RING][:n].cpu().numpy(), tick0 + t)
                    assert T._eq(env.GetState(), replay.s), (t, T._first_diff(env.GetState(), replay.s))
                    assert T._eq(out.Observation, obs.T), (t, T._first_diff(out.Observation.T, obs))
                    assert T._eq(out.Reward, rw) and T._eq(env.GetArray("done"), db), t
        else:
            env.RolloutDevice(ring, STEPS, stride, RING)
        env.Sync()
        out = env.Read()
        return env.GetState(), out.Observation.copy(), out.Reward.copy(), env.GetArray("done"), env.Tick - tick0


@pytest.mark.gpu
@pytest.mark.parametrize("env,n,count,lane_offset", _cases())
def test_full_workgroup_body_equals_the_oracle_and_the_scalar_form(gpu_pkg, oracle, env, n, count, lane_offset):
    import torch
    if not T._ORACLE:
        T._ORACLE.append(oracle)
    w = M.wide_of(env)
    rf = 1 if M.has_reset_form1(env, w) else 0
    wide = dict(vec=w, sequential_lanes=1, reset_form=rf)
    r = _recipe(env, n, lane_offset, w)
    rng = np.random.default_rng(n * 131 + count * 7 + lane_offset % 1009 + len(env))
    s0 = _start(env, n, count, rng)
    stride = (n + 63) // 64 * 64                                            # every action slice and observation row 16-byte aligned
    acts = np.zeros((RING, stride), np.float32 if M.ENVS[env]["box"] else np.int32)
    for k in range(RING):
        acts[k, :n] = T._actions(r, rng, n)
    ring = torch.from_numpy(acts).cuda()
    torch.cuda.synchronize()

    if env != "Pendulum":                                                   # the start state does what it is built for, on THESE inputs
        fin0 = T.Replay(oracle, r, s0.astype(np.float64 if r["f64"] else np.float32)).step(acts[0, :n], 0)[3]
        assert int(fin0[:64 * w].sum()) == count, (int(fin0[:64 * w].sum()), count)

    # reference 2: the scalar form (per-lane addressing, the per-thread reset loop) on the same inputs, itself held to the oracle
    s0r = s0.astype(np.float64 if r["f64"] else np.float32)
    ref = _run(gpu_pkg, torch, r, dict(vec=1, sequential_lanes=1, reset_form=0), f"step_kernel<{env},1,true,false,", "in_place", "step",
               s0, ring, stride, T.Replay(oracle, r, s0r))
    assert ref[4] == STEPS
    for buffers in BUFFERS:
        for path in PATHS:
            # reference 1: the oracle's batched auto-reset step, every step, on the per-step path of every buffer arrangement
            replay = T.Replay(oracle, r, s0r) if path == "step" else None
            got = _run(gpu_pkg, torch, r, wide, f"step_kernel<{env},{w},true,false,", buffers, path, s0, ring, stride, replay)
            for a, b in zip(ref[:4], got[:4]):
                assert T._eq(a, b), (buffers, path, T._first_diff(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)))
            assert got[4] == STEPS, (buffers, path)                          # the device tick after the run


def test_start_states_finish_the_counts_they_name(oracle):
    """The start states above are only worth something if the first wave finishes exactly `count` sub-lanes at step 0 (CPU only: the
    oracle's step on the states the GPU test builds)."""
    for env in ("CartPole", "MountainCar"):
        wave = 64 * M.wide_of(env)
        for n in SIZES:
            for count in _counts(env, n):
                rng = np.random.default_rng(1)
                s0 = _start(env, n, count, rng)
                r = _recipe(env, n, 0, 4)
                for a in range(M.ENVS[env]["nvals"]):
                    _, _, _, d = oracle.env_step(r["gym"], s0, np.full(n, a, np.int32), sbd=None, dtype=np.float32)
                    assert int(np.asarray(d)[:wave].astype(bool).sum()) == count, (env, n, count, a)
