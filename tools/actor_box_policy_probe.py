"""Times a Box actor's policies (gym.net_amd/csrc/actor_box_policy.hip) against the default policy (actor_box.hip) with HIP events in one
process: Pendulum and MountainCarContinuous float32, 2^20 lanes by default, auto-reset, the network [history * obs_dim, 50, 20, 1]
(history 4), epsilon 1 — every lane explores, so every lane pays the policy's transcendentals: the worst case.

    python tools/actor_box_policy_probe.py [--lanes 20] [--reps 20] [--steps 256] [--out profiles/actor_box_policy_probe.txt]

Rows per env and policy (per vector step, median of --reps timings; the fused rollout: of max(3, reps / 4) launches of --steps steps):
  box_act              gymnet_vecenv_actor_box_act_device alone
  fused                one GYMNET_ACTIONS_ACTOR rollout on a plain auto-reset handle
for the default policy ("clamp", "sample") — actor_box.hip's kernels, the comparison — and for ("tanh", "gaussian", 0.3), on the same
handle in the same run, the policies alternating.  Needs a GPU; no fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENVS = [("Pendulum-v1", 3), ("MountainCarContinuous-v0", 2)]
HISTORY, HIDDEN, EPS = 4, [50, 20], 1.0
POLICIES = [("clamp", "sample", 0.0), ("tanh", "gaussian", 0.3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=20, help="log2 lane count")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if pkg.device_count() < 1:
        raise SystemExit("actor_box_policy_probe: no GPU")
    n, T = 1 << args.lanes, args.steps
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    lines, rows = [], {}

    def timed(fn, reps):
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return float(np.median(ts))

    lines.append(f"lanes 2^{args.lanes} float32 auto-reset, actor [{HISTORY} * obs_dim, 50, 20, 1] (history {HISTORY}), epsilon {EPS}, "
                 f"fused T = {T}; us per vector step")
    for name, O in ENVS:
        torch.manual_seed(0)
        seq = torch.nn.Sequential(torch.nn.Linear(HISTORY * O, 50), torch.nn.ReLU(), torch.nn.Linear(50, 20), torch.nn.ReLU(), torch.nn.Linear(20, 1))
        with pkg.VectorEnv(name, n, seed=1, auto_reset=True, stream=stream.cuda_stream) as env:
            env.Reset()
            actor = env.Actor(seq, history=HISTORY)
            acts = torch.empty(n, dtype=torch.float32, device="cuda")
            for t in range(5):
                actor.Step(EPS, 7, t)
            for policy in POLICIES + POLICIES:                   # each policy twice, alternating: the second pass is the one kept
                actor.SetPolicy(*policy)
                key = "/".join(policy[:2])
                act_us = timed(lambda: actor.Act(EPS, 7, 5, out=acts), args.reps)
                fused_us = timed(lambda: env.RolloutFusedDevice(None, T, actions="actor", epsilon=EPS, action_seed=7, action_tick0=0),
                                 max(3, args.reps // 4)) / T
                rows.setdefault(name, {})[key] = {"act_us": round(act_us, 2), "fused_us": round(fused_us, 2)}
            for policy in POLICIES:
                key = "/".join(policy[:2])
                r = rows[name][key]
                lines.append(f"{name:26s} {key:16s} sigma {policy[2]:.1f}   box_act {r['act_us']:8.2f} us   fused, T = {T} {r['fused_us']:8.2f} us")
            d, p = (rows[name]["/".join(q[:2])] for q in POLICIES)
            lines.append(f"{name:26s} tanh/gaussian - clamp/sample: box_act {p['act_us'] - d['act_us']:+.2f} us ({p['act_us'] / d['act_us']:.3f}x)   "
                         f"fused {p['fused_us'] - d['fused_us']:+.2f} us ({p['fused_us'] / d['fused_us']:.3f}x)")
    text = "\n".join(lines) + "\n" + json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, "lanes": n, "steps": T, "epsilon": EPS,
                                                 "rows": rows}) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
