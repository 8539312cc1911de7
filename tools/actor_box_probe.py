"""Times the Box actor (gym.net_amd/csrc/actor_box.hip) with HIP events in one process: Pendulum and MountainCarContinuous float32,
2^20 lanes by default, auto-reset, the network [history * obs_dim, 50, 20, 1] (history 4), epsilon 0.1 — and, as the yardstick for
MountainCarContinuous, the Discrete actor on MountainCar with the same hidden widths (the nets differ in the last layer only: 3 outputs
against 1), on the same library in the same process.

    python tools/actor_box_probe.py [--lanes 20] [--reps 20] [--steps 256] [--runs 3] [--out profiles/actor_box_probe.txt]

Rows per env (per vector step, median of --reps timings):
  act                  gymnet_vecenv_actor_box_act_device (actor_act_device on MountainCar) alone
  unfused loop         act + step_device + push
  fused                one GYMNET_ACTIONS_ACTOR rollout of --steps steps: plain auto-reset handle
  fused records        the same on a trainer-shaped handle (EPISODE_STATS, max_episode_steps 200) keeping compact episode records
  torch path           history (the actor's own buffer, viewed by torch) -> nn.Sequential -> clamp -> torch.where(coin, sample, greedy) ->
                       StepDevice (Box envs; the coin and the sample are the engine's own streams' stand-ins: torch.rand draws, which cost
                       no more), history upkeep not included: it favours torch
The fused lean row is measured --runs times per env (fresh handle each), so that the MountainCarContinuous - MountainCar difference can be
read against the run-to-run spread.  Needs a GPU; no fallback."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENVS = [("Pendulum-v1", 3, 1), ("MountainCarContinuous-v0", 2, 1), ("MountainCar-v0", 2, 3)]      # name, obs_dim, last width
HISTORY, HIDDEN, EPS = 4, [50, 20], 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=20, help="log2 lane count")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if pkg.device_count() < 1:
        raise SystemExit("actor_box_probe: no GPU")
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

    def row(env, name, us, key):
        lines.append(f"{env:26s} {name:40s} {us:9.2f} us")
        rows.setdefault(env, {})[key] = round(us, 2)

    def fused(env, ep=None):
        return timed(lambda: env.RolloutFusedDevice(None, T, actions="actor", epsilon=EPS, action_seed=7, action_tick0=0, episodes=ep),
                     reps=max(3, args.reps // 4)) / T

    lines.append(f"lanes 2^{args.lanes} float32 auto-reset, actor [{HISTORY} * obs_dim, 50, 20, last] (history {HISTORY}), epsilon {EPS}, "
                 f"fused T = {T}; us per vector step")
    for name, O, last in ENVS:
        torch.manual_seed(0)
        widths = [HISTORY * O] + HIDDEN + [last]
        seq = torch.nn.Sequential(torch.nn.Linear(widths[0], 50), torch.nn.ReLU(), torch.nn.Linear(50, 20), torch.nn.ReLU(), torch.nn.Linear(20, last))
        box = last == 1
        with pkg.VectorEnv(name, n, seed=1, auto_reset=True, stream=stream.cuda_stream) as env:
            env.Reset()
            actor = env.Actor(seq, history=HISTORY)
            acts = torch.empty(n, dtype=torch.float32 if box else torch.int32, device="cuda")
            tick = [0]

            def step_loop():
                tick[0] += 1
                actor.Step(EPS, 7, tick[0])

            for _ in range(5):
                step_loop()
            row(name, "box_act" if box else "act", timed(lambda: actor.Act(EPS, 7, tick[0], out=acts)), "act_us")
            row(name, "unfused loop (act+step+push)", timed(step_loop), "unfused_us")
            row(name, f"fused, T = {T}", fused(env), "fused_us")
            if box:
                vp, vs, vl = C.c_void_p(), C.c_int64(), C.c_int32()
                env._lib.gymnet_vecenv_actor_view(env._h, C.byref(vp), C.byref(vs), C.byref(vl))

                class _View:
                    __cuda_array_interface__ = {"shape": (HISTORY, O, int(vs.value)), "typestr": "<f4", "data": (int(vp.value), False),
                                                "version": 2, "strides": None}
                hist = torch.as_tensor(_View(), device="cuda")
                dseq = seq.to("cuda")
                low, high = float(env.ActionSpace.Low[0]), float(env.ActionSpace.High[0])

                def torch_step():
                    x = hist.reshape(HISTORY * O, -1)[:, :n].t()
                    greedy = dseq(x)[:, 0].clamp(low, high)
                    coin = torch.rand(n, device="cuda") <= EPS
                    sample = low + (high - low) * torch.rand(n, device="cuda")
                    acts.copy_(torch.where(coin, sample, greedy))
                    env.StepDevice(acts)

                with torch.no_grad():
                    torch_step()
                    row(name, "torch path (Sequential+clamp+where+step)", timed(torch_step), "torch_us")
        with pkg.VectorEnv(name, n, seed=1, auto_reset=True, episode_stats=True, max_episode_steps=200, stream=stream.cuda_stream) as env:
            env.Reset()
            actor = env.Actor(seq, history=HISTORY)
            cap = 1 << 22
            ep = dict(step=torch.empty(cap, dtype=torch.int32, device="cuda"), lane=torch.empty(cap, dtype=torch.int32, device="cuda"),
                      ret=torch.empty(cap, dtype=torch.float32, device="cuda"), length=torch.empty(cap, dtype=torch.int32, device="cuda"),
                      capacity=cap, count=torch.zeros(2, dtype=torch.int32, device="cuda"))
            row(name, f"fused trainer-shaped + records, T = {T}", fused(env, ep), "fused_records_us")
    # the yardstick: the lean fused rollout, --runs fresh handles per env, alternating
    runs = {name: [] for name, _, _ in ENVS[1:]}
    for _ in range(args.runs):
        for name, O, last in ENVS[1:]:
            torch.manual_seed(0)
            seq = torch.nn.Sequential(torch.nn.Linear(HISTORY * O, 50), torch.nn.ReLU(), torch.nn.Linear(50, 20), torch.nn.ReLU(), torch.nn.Linear(20, last))
            with pkg.VectorEnv(name, n, seed=1, auto_reset=True, stream=stream.cuda_stream) as env:
                env.Reset()
                env.Actor(seq, history=HISTORY)
                fused(env)
                runs[name].append(round(fused(env), 2))
    for name, v in runs.items():
        lines.append(f"{name:26s} fused, {args.runs} runs: {v}  median {np.median(v):.2f}  spread {max(v) - min(v):.2f} us")
    box_v, disc_v = runs["MountainCarContinuous-v0"], runs["MountainCar-v0"]
    lines.append(f"MountainCarContinuous - MountainCar (medians): {np.median(box_v) - np.median(disc_v):+.2f} us")
    for name, _, last in ENVS[:2]:
        r = rows[name]
        lines.append(f"{name}: fused beats the torch path {r['torch_us'] / r['fused_us']:.2f}x (records: {r['torch_us'] / r['fused_records_us']:.2f}x)")
    text = "\n".join(lines) + "\n" + json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, "lanes": n, "steps": T, "rows": rows,
                                                 "fused_runs": runs}) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
