"""The one-step kernels receive their first-use argument words as flat (preloaded) kernel arguments and the rest of the StepArgsT behind
them (csrc/kernels.hpp StepKernelFn; step_kernels.hpp launch_step_kernel splits, hot_step_args joins).  A word that went to the wrong
place would show as a wrong address, guard, tick or parity — so every form of every env is run at the sizes where those matter and
compared, bit for bit, with the oracle's batched auto-reset step (the replay of tests/test_gpu_instantiation_matrix.py) and across the
three launch paths that pass the words differently: one StepDevice launch per step, RolloutDevice's back-to-back launches, and
RolloutDevice replaying a captured hipGraph (which froze the words).

  envs      the four float32 envs and float64 CartPole
  forms     scalar; the wide lanes with reset form 0 and 1; step_kernel_pipe items 2 and 5; step_kernel_pipe2 items 2 and 4
  buffers   in place, GYMNET_FLAG_DOUBLE_BUFFER, external observation buffers
  paths     StepDevice per step, RolloutDevice eager, RolloutDevice with graph=1; ring 2, 8 steps
  sizes     1 lane, one exact workgroup of the form, one workgroup + 3 lanes (the guarded tail); for the sliced pipe2 form one slice
            boundary (one resident generation + a ragged second slice)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _instantiation_matrix as M  # noqa: E402
import test_gpu_instantiation_matrix as T  # noqa: E402  (its Replay and start states; only the module object is imported)

pytestmark = pytest.mark.gpu
SEED, STEPS, RING, BLOCK = 0x5EED, 8, 2, 256
BUFFERS = ("in_place", "double_buffer", "external")
PATHS = ("step", "rollout", "graph")


def _forms(env):
    """(id, launch policy, lanes per workgroup, expected KernelName prefix, expected suffix) of every form the env has."""
    e, w = M.ENVS[env], M.wide_of(env)
    f = [("scalar", dict(vec=1, sequential_lanes=1, reset_form=0), BLOCK, f"step_kernel<{env},1,true,false,", ",0>"),
         (f"wide{w}_rf0", dict(vec=w, sequential_lanes=1, reset_form=0), BLOCK * w, f"step_kernel<{env},{w},true,false,", ",0>")]
    if M.has_reset_form1(env, w):
        f.append((f"wide{w}_rf1", dict(vec=w, sequential_lanes=1, reset_form=1), BLOCK * w, f"step_kernel<{env},{w},true,false,", ",1>"))
    if e["pipe_lanes"]:
        f += [(f"pipe{k}", dict(vec=1, sequential_lanes=k), BLOCK * k, f"step_kernel_pipe<{env},{k},true,", ">") for k in (2, 5)]
    if e["pipe_pairs"]:
        f += [(f"pipe2_{k}", dict(vec=2, sequential_lanes=k), 2 * k * BLOCK, f"step_kernel_pipe2<{env},{k},true,", ">") for k in (2, 4)]
    return f


def _cases():
    out = []
    for env in ("CartPole", "MountainCar", "Pendulum", "Acrobot", "CartPole64"):
        for fid, policy, group, prefix, suffix in _forms(env):
            sizes = [1, group, group + 3]
            if fid.startswith("pipe2") and not M.ENVS[env]["split_reset"]:
                sizes = [group, 2 * group]                       # the pair form without the deferred reset runs whole groups only
            if fid == "pipe2_4" and M.ENVS[env]["split_reset"]:
                sizes.append(1024 // 4 * 2 * group + group + 3)  # pipe2_chunks: one resident generation, then a ragged second slice
            for n in sizes:
                out.append(pytest.param(env, policy, n, prefix, suffix, id=f"{env}-{fid}-n{n}"))
    return out


def _recipe(env, policy, n):
    e = M.ENVS[env]
    return dict(env=env, gym=e["gym"], n=n, f64=e["f64"], vec=policy["vec"], items=policy["sequential_lanes"], lane_seeds=False, auto_reset=True,
                episode_stats=False, max_episode_steps=0, final_obs=False, lane_offset=0, done_list=False)


def _run(gpu_pkg, torch, r, policy, buffers, path, s0, ring, stride, prefix, suffix, replay=None):
    """8 steps on one fresh handle; returns (state, observation, reward, done, tick).  replay: compare every step with the oracle."""
    n, dt = r["n"], (np.float64 if r["f64"] else np.float32)
    tdt = torch.float64 if r["f64"] else torch.float32
    kw, keep = {}, []
    if buffers == "double_buffer":
        kw["double_buffer"] = True
    elif buffers == "external":
        odim = {"CartPole": 4, "CartPole64": 4, "MountainCar": 2, "Pendulum": 3, "Acrobot": 6}[r["env"]]
        ext = torch.zeros(odim * stride, dtype=tdt, device="cuda")
        keep.append(ext)
        kw.update(ext_obs=ext.data_ptr(), ext_obs_stride=stride)
        torch.cuda.synchronize()                                        # the handle launches on a stream of its own
    with gpu_pkg.VectorEnv(r["gym"], n, seed=SEED, auto_reset=True, dtype=dt, **kw) as env:
        env.SetLaunchPolicy(graph=1 if path == "graph" else 0, **policy)
        name = env.KernelName()
        assert name.startswith(prefix) and name.split(" x ")[0].endswith(suffix), (name, prefix, suffix)
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
        assert env.KernelName() == name
        return env.GetState(), out.Observation.copy(), out.Reward.copy(), env.GetArray("done"), env.Tick - tick0


@pytest.mark.parametrize("env,policy,n,prefix,suffix", _cases())
def test_every_form_equals_the_oracle_on_every_launch_path(gpu_pkg, oracle, golden, env, policy, n, prefix, suffix):
    import torch
    if not T._ORACLE:
        T._ORACLE.append(oracle)
    r = _recipe(env, policy, n)
    rng = np.random.default_rng(n * 31 + len(prefix))
    s0, a0, must, keep = T._start(r, golden, rng)
    stride = (n + 63) // 64 * 64                                        # every action slice and observation row 16-byte aligned
    acts = np.zeros((RING, stride), np.float32 if M.ENVS[env]["box"] else np.int32)
    for k in range(RING):
        acts[k, :n] = T._actions(r, rng, n)
    if a0 is not None:
        acts[0, :n] = np.where(a0 >= 0, a0, acts[0, :n])
    ring = torch.from_numpy(acts).cuda()
    torch.cuda.synchronize()
    results = {}
    for buffers in BUFFERS:
        for path in PATHS:
            # the oracle's batched auto-reset step, every step, on the per-step path; every other combination must equal that run
            replay = T.Replay(oracle, r, s0.astype(np.float64 if r["f64"] else np.float32)) if (buffers, path) == ("in_place", "step") else None
            results[buffers, path] = _run(gpu_pkg, torch, r, policy, buffers, path, s0, ring, stride, prefix, suffix, replay)
    ref = results["in_place", "step"]
    assert ref[4] == STEPS
    for key, got in results.items():
        for a, b in zip(ref[:4], got[:4]):
            assert T._eq(a, b), (key, T._first_diff(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)))
        assert got[4] == STEPS, key                                     # the device tick after the run
