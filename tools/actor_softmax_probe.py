"""Times a Discrete actor's softmax exploration (gym.net_amd/csrc/actor_softmax.hip) against the default setting (actor.hip's kernels) with
HIP events in one process: CartPole with the runner's net [16, 50, 20, 2] and Acrobot with [24, 50, 20, 3] (history 4), float32, 2^20
lanes by default, auto-reset, epsilon 1 — every lane explores, so every lane pays the softmax: the worst case.

    python tools/actor_softmax_probe.py [--lanes 20] [--reps 7] [--steps 256] [--passes 2] [--out profiles/actor_softmax_probe.txt]

Rows per env and setting (per vector step, median of --reps timings, at least five):
  act                  gymnet_vecenv_actor_act_device alone
  fused                one GYMNET_ACTIONS_ACTOR rollout of --steps steps on a plain auto-reset handle
for the default ("uniform") — the comparison — and for ("softmax", 1.0), on the same handle, alternating.  The whole measurement runs
--passes times (a fresh handle each), so a run-to-run spread exists: the table gives each pass and, per row, the spread between the
passes beside the difference between the settings.  Needs a GPU; no fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENVS = [("CartPole-v1", 4, 2), ("Acrobot-v1", 6, 3)]
HISTORY, HIDDEN, EPS = 4, [50, 20], 1.0
SETTINGS = [("uniform", 1.0), ("softmax", 1.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=20, help="log2 lane count")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps = max(5, args.reps)
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if pkg.device_count() < 1:
        raise SystemExit("actor_softmax_probe: no GPU")
    n, T = 1 << args.lanes, args.steps
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)

    def timed(fn):
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return float(np.median(ts))

    lines = [f"lanes 2^{args.lanes} float32 auto-reset, actor [{HISTORY} * obs_dim, 50, 20, A] (history {HISTORY}), epsilon {EPS}, fused T = {T}, "
             f"median of {reps}; us per vector step; {args.passes} passes"]
    rows = {}
    for p in range(args.passes):
        for name, O, A in ENVS:
            torch.manual_seed(0)
            seq = torch.nn.Sequential(torch.nn.Linear(HISTORY * O, 50), torch.nn.ReLU(), torch.nn.Linear(50, 20), torch.nn.ReLU(), torch.nn.Linear(20, A))
            with pkg.VectorEnv(name, n, seed=1, auto_reset=True, stream=stream.cuda_stream) as env:
                env.Reset()
                actor = env.Actor(seq, history=HISTORY)
                acts = torch.empty(n, dtype=torch.int32, device="cuda")
                for t in range(5):
                    actor.Step(EPS, 7, t)
                for setting in SETTINGS + SETTINGS:                  # each setting twice, alternating: the second round is the one kept
                    actor.SetExploration(*setting)
                    act_us = timed(lambda: actor.Act(EPS, 7, 5, out=acts))
                    fused_us = timed(lambda: env.RolloutFusedDevice(None, T, actions="actor", epsilon=EPS, action_seed=7, action_tick0=0)) / T
                    rows.setdefault(name, {}).setdefault(setting[0], [None] * args.passes)[p] = {"act_us": round(act_us, 2), "fused_us": round(fused_us, 2)}
    for name, _, _ in ENVS:
        for key, _ in SETTINGS:
            for p, r in enumerate(rows[name][key]):
                lines.append(f"{name:14s} {key:8s} pass {p + 1}   act {r['act_us']:8.2f} us   fused, T = {T} {r['fused_us']:8.2f} us")
        for what in ("act_us", "fused_us"):
            d = np.array([r[what] for r in rows[name]["uniform"]])
            s = np.array([r[what] for r in rows[name]["softmax"]])
            lines.append(f"{name:14s} {what[:-3]:5s} softmax - uniform per pass: " + ", ".join(f"{x:+.2f} us ({y:.3f}x)" for x, y in zip(s - d, s / d)) +
                         f"   spread between passes: uniform {d.max() - d.min():.2f} us, softmax {s.max() - s.min():.2f} us")
    text = "\n".join(lines) + "\n" + json.dumps({"device": torch.cuda.get_device_name(0), "reps": reps, "lanes": n, "steps": T, "epsilon": EPS,
                                                 "passes": args.passes, "rows": rows}) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
