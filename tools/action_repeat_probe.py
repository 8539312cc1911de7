"""Times frame skip (gym.net_amd/csrc/action_repeat.hip) with HIP events in one process: CartPole and Pendulum float32, 2^20 lanes by
default, auto-reset, R = 2, 4, 8 sub-steps per decision.

    python tools/action_repeat_probe.py [--lanes 20] [--reps 30] [--steps 64] [--out profiles/action_repeat_probe.txt]

Per env and R, us per DECISION (median of --reps timings):
  yardstick #1..#3     R single steps as the step path runs them: RolloutDevice(actions, R, 0, 1), the graph-replayed one-step launches —
                       taken three times, alternating with the new call, so the claim can be read against its own run-to-run spread
  step_repeat #1..#3   StepRepeatDevice(actions, R - 1): one launch
  fused                RolloutFusedDevice(ring, T, repeat=R - 1) per decision, T = --steps, against
  fused yardstick      RolloutFusedDevice over T * R steps with each action R times in the ring (the same actions, no frame-skip semantics)
The claim under test: one decision costs less than R single-step launches for every R >= 2, by more than the yardstick's spread.
Needs a GPU; no fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENVS = [("CartPole-v1", False), ("Pendulum-v1", True)]
REPEATS = (2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=20, help="log2 lane count")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if pkg.device_count() < 1:
        raise SystemExit("action_repeat_probe: no GPU")
    n, T = 1 << args.lanes, args.steps
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    lines, rows = [], {}

    def timed(fn, reps=None):
        ts = []
        for _ in range(reps or args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return float(np.median(ts))

    lines.append(f"lanes 2^{args.lanes} float32 auto-reset; us per decision of R sub-steps (median of {args.reps}); fused T = {T} decisions")
    for name, box in ENVS:
        gen = torch.Generator(device="cuda").manual_seed(3)
        with pkg.VectorEnv(name, n, seed=1, auto_reset=True, stream=stream.cuda_stream) as env:
            env.Reset()
            if box:
                acts = torch.rand(n, generator=gen, device="cuda") * 4 - 2
            else:
                acts = torch.randint(0, 2, (n,), generator=gen, device="cuda", dtype=torch.int32)
            for R in REPEATS:
                ring = acts.repeat(8, 1).contiguous()                       # 8 decisions' actions (the same row: timing only)
                ring_r = ring.repeat_interleave(R, dim=0).contiguous()      # each action R times: the fused yardstick's ring
                stream.synchronize()
                for _ in range(3):                                          # warm-up: graph capture, first launches
                    env.RolloutDevice(acts, R, 0, 1)
                    env.StepRepeatDevice(acts, R - 1)
                yard, held = [], []
                for _ in range(3):
                    yard.append(timed(lambda: env.RolloutDevice(acts, R, 0, 1)))
                    held.append(timed(lambda: env.StepRepeatDevice(acts, R - 1)))
                few = max(3, args.reps // 6)
                env.RolloutFusedDevice(ring, T, n, 8, repeat=R - 1)
                env.RolloutFusedDevice(ring_r, T * R, n, 8 * R)
                fused = timed(lambda: env.RolloutFusedDevice(ring, T, n, 8, repeat=R - 1), reps=few) / T
                fused_y = timed(lambda: env.RolloutFusedDevice(ring_r, T * R, n, 8 * R), reps=few) / T
                spread = max(yard) - min(yard)
                gain = min(yard) - max(held)
                verdict = "holds" if gain > spread else "FAILS"
                lines.append(f"{name:12s} R = {R}  yardstick {' '.join(f'{v:8.2f}' for v in yard)}   step_repeat {' '.join(f'{v:8.2f}' for v in held)}"
                             f"   worst gain {gain:+7.2f} us vs spread {spread:5.2f}: the claim {verdict}"
                             f"   | fused {fused:7.2f}  fused yardstick {fused_y:7.2f}")
                rows[f"{name} R={R}"] = {"yardstick_us": [round(v, 2) for v in yard], "step_repeat_us": [round(v, 2) for v in held],
                                         "fused_us": round(fused, 2), "fused_yardstick_us": round(fused_y, 2), "claim": verdict}
    text = "\n".join(lines) + "\n" + json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, "lanes": n, "steps": T, "rows": rows}) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
