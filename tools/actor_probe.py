"""Times the actor (gym.net_amd/csrc/actor.hip) with HIP events in one process: CartPole float32, 2^20 lanes by default, auto-reset, the
Parameters runner's network 16-50-20-2 (history 4), epsilon 0.1.

    python tools/actor_probe.py [--lanes 20] [--reps 20] [--steps 256] [--out profiles/actor_probe.txt]

Rows:
  act                  gymnet_vecenv_actor_act_device alone
  push                 gymnet_vecenv_actor_push_device alone (after a StepDevice outside the window)
  step_device          one StepDevice launch, the reference point
  unfused loop         act + step_device + push, per step
  fused                one GYMNET_ACTIONS_ACTOR rollout of --steps steps, per vector step: plain auto-reset handle, and a trainer-shaped
                       handle (EPISODE_STATS, max_episode_steps 500) keeping compact episode records
  torch path           history (the actor's own buffer, viewed by torch) -> nn.Sequential -> argmax -> ComposeActionsDevice -> StepDevice,
                       per step (history upkeep not included: it favours torch)
Every figure also as a fraction of the 157.3 TF FP32 spec: 2 * 1840 FLOP per env-step / time.  Needs a GPU; no fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SPEC = 157.3e12
WIDTHS = [16, 50, 20, 2]


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
        raise SystemExit("actor_probe: no GPU")
    n = 1 << args.lanes
    flops = 2.0 * sum(WIDTHS[i] * WIDTHS[i + 1] for i in range(len(WIDTHS) - 1)) * n
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    torch.manual_seed(0)
    seq = torch.nn.Sequential(torch.nn.Linear(16, 50), torch.nn.ReLU(), torch.nn.Linear(50, 20), torch.nn.ReLU(), torch.nn.Linear(20, 2))
    lines, rows = [], {}

    def timed(fn, before=None, reps=None):
        ts = []
        for _ in range(reps or args.reps):
            if before:
                before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return float(np.median(ts))

    def frac(us):
        return flops / (us * 1e-6) / SPEC

    def row(name, us, key, network=True):
        if network:
            lines.append(f"{name:44s} {us:9.2f} us  = {flops / (us * 1e-6) / 1e12:6.1f} TF = {frac(us):5.3f} of the 157.3 TF FP32 spec")
        else:
            lines.append(f"{name:44s} {us:9.2f} us  (no network evaluation)")
        rows[key] = round(us, 2)

    lines.append(f"lanes 2^{args.lanes} CartPole float32 auto-reset, actor {'-'.join(map(str, WIDTHS))} (history 4), epsilon 0.1, "
                 f"{flops / n:.0f} FLOP per env-step")
    with pkg.VectorEnv("CartPole-v1", n, seed=1, auto_reset=True, stream=stream.cuda_stream) as env:
        env.Reset()
        actor = env.Actor(seq, history=4)
        acts = torch.empty(n, dtype=torch.int32, device="cuda")
        tick = [0]

        def step_loop():
            tick[0] += 1
            actor.Step(0.1, 7, tick[0])

        for _ in range(5):
            step_loop()
        row("act", timed(lambda: actor.Act(0.1, 7, tick[0], out=acts)), "act_us")
        row("push", timed(actor.Push, before=lambda: env.StepDevice(acts)), "push_us", network=False)
        actor.Reset()
        row("step_device", timed(lambda: env.StepDevice(acts)), "step_us", network=False)
        actor.Reset()
        row("unfused loop (act+step+push)", timed(step_loop), "unfused_us")
        T = args.steps
        us = timed(lambda: env.RolloutFusedDevice(None, T, actions="actor", epsilon=0.1, action_seed=7, action_tick0=0), reps=max(3, args.reps // 4)) / T
        row(f"fused, T = {T}, per vector step", us, "fused_us")
        # the torch path: history -> Sequential -> argmax -> compose -> step
        import ctypes as C
        vp, vs, vl = C.c_void_p(), C.c_int64(), C.c_int32()
        env._lib.gymnet_vecenv_actor_view(env._h, C.byref(vp), C.byref(vs), C.byref(vl))

        class _View:
            __cuda_array_interface__ = {"shape": (4, 4, int(vs.value)), "typestr": "<f4", "data": (int(vp.value), False), "version": 2,
                                        "strides": None}
        hist = torch.as_tensor(_View(), device="cuda")
        dseq = seq.to("cuda")
        greedy = torch.empty(n, dtype=torch.int32, device="cuda")

        def torch_step():
            x = hist.reshape(16, -1)[:, :n].t()
            greedy.copy_(dseq(x).argmax(dim=1))
            env.ComposeActionsDevice(greedy, 0.1, acts, seed=7, tick=0)
            env.StepDevice(acts)

        with torch.no_grad():
            torch_step()
            row("torch path (Sequential+argmax+compose+step)", timed(torch_step), "torch_us")
    with pkg.VectorEnv("CartPole-v1", n, seed=1, auto_reset=True, episode_stats=True, max_episode_steps=500, stream=stream.cuda_stream) as env:
        env.Reset()
        actor = env.Actor(seq, history=4)
        T = args.steps
        cap = 1 << 22
        ep = dict(step=torch.empty(cap, dtype=torch.int32, device="cuda"), lane=torch.empty(cap, dtype=torch.int32, device="cuda"),
                  ret=torch.empty(cap, dtype=torch.float32, device="cuda"), length=torch.empty(cap, dtype=torch.int32, device="cuda"),
                  capacity=cap, count=torch.zeros(2, dtype=torch.int32, device="cuda"))
        us = timed(lambda: env.RolloutFusedDevice(None, T, actions="actor", epsilon=0.1, action_seed=7, action_tick0=0, episodes=ep),
                   reps=max(3, args.reps // 4)) / T
        row(f"fused trainer-shaped + records, T = {T}", us, "fused_records_us")
    text = "\n".join(lines) + "\n" + json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, "lanes": n, **rows}) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
