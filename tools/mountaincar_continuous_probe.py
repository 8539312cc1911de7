#!/usr/bin/env python3
"""Times MountainCarContinuous-v0 next to MountainCar-v0 in ONE process on one device (profiles/mountaincar_continuous.txt):
  - the one-step launch (StepDevice, auto-reset, the handle's default launch policy) at 2^19, 5 * 2^18, 2^20 and 2^22 lanes, the two envs
    interleaved rep after rep, HIP-event time per step; the kernel each handle launches (KernelName);
  - the fused rollout at 2^20 lanes: actions from a 64-slice ring, and actions drawn in the kernel (ActionSpace.Sample()).
    python tools/mountaincar_continuous_probe.py [--steps K] [--reps R]        prints one JSON object
Run under `rocprofv3 --kernel-trace --stats -- python tools/mountaincar_continuous_probe.py --steps 200 --reps 1` for the kernel table
(a separate run: the tracer's own overhead is not in the event times)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

ENVS = ("MountainCar-v0", "MountainCarContinuous-v0")
SIZES = (1 << 19, 5 << 18, 1 << 20, 1 << 22)
RING = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    torch.cuda.set_stream(st)

    def timed(fn, steps):
        fn(min(steps, 100))                                                 # warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); fn(steps); e1.record(st); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / steps                            # us per vector step

    out = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "reps": args.reps, "step": {}, "fused_2^20": {}}
    for n in SIZES:
        envs, acts, us = {}, {}, {name: [] for name in ENVS}
        for name in ENVS:
            env = pkg.VectorEnv(name, n, seed=1, auto_reset=True, stream=st.cuda_stream)
            a = torch.empty((RING, n), dtype=torch.float32 if isinstance(env.ActionSpace, pkg.Box) else torch.int32, device=dev)
            for t in range(RING):
                env.SampleActionsDevice(a[t], seed=2, tick=t)
            env.ResetDevice()
            envs[name], acts[name] = env, a
        for _ in range(args.reps):                                          # interleaved: both envs see the same box state
            for name in ENVS:
                env, a = envs[name], acts[name]
                us[name].append(timed(lambda k: [env.StepDevice(a[t % RING]) for t in range(k)], args.steps))
        for name in ENVS:
            out["step"].setdefault(name, {})[str(n)] = {"kernel": envs[name].KernelName(), "us_per_step_median": statistics.median(us[name]),
                                                        "us_per_step_all": us[name]}
            envs[name].Close()
    n = 1 << 20
    for name in ENVS:
        env = pkg.VectorEnv(name, n, seed=1, auto_reset=True, stream=st.cuda_stream)
        a = torch.empty((RING, n), dtype=torch.float32 if isinstance(env.ActionSpace, pkg.Box) else torch.int32, device=dev)
        for t in range(RING):
            env.SampleActionsDevice(a[t], seed=2, tick=t)
        env.ResetDevice()
        res = {}
        for mode in ("ring", "sample"):
            def run(k, mode=mode):
                for c in range(k // RING):                                  # RING steps per launch
                    if mode == "ring":
                        env.RolloutFusedDevice(a, RING, n, RING)
                    else:
                        env.RolloutFusedDevice(None, RING, actions="sample", action_seed=3, action_tick0=c * RING)
            res[mode] = statistics.median(timed(run, max(args.steps // RING, 1) * RING) for _ in range(args.reps))
        out["fused_2^20"][name] = {"us_per_step_ring": res["ring"], "us_per_step_sample": res["sample"]}
        env.Close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
