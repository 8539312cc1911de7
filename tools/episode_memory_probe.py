"""Times the episode memory (gym.net_amd/csrc/episode_memory.hip) with HIP events in one process: CartPole float32, 2^20 lanes by default,
auto-reset with max_episode_steps 500, capacity 100, max_length 500, history 4 (the Parameters runner's shape).

    python tools/episode_memory_probe.py [--lanes 20] [--reps 20] [--out profiles/episode_memory_probe.txt]

Rows:
  step_device          one StepDevice launch (sampled actions), the reference point
  push, no admission   a push whose done bytes are all zero (no episode ends: the ring traffic alone, push + empty merge launch)
  push, steady state   a push with the handle's own done bytes once the pool is full (few admissions)
  push, warm-up        each of the first pushes after config, when every ended episode is a candidate
  dataset build        gymnet_vecenv_memory_dataset_device for the kept episodes: params rows and BINARY_F32 40 x 20 frames
The push's bytes per lane (read obs, action, reward, done, open length and return; write the ring's obs, action and reward, the length and
return) over its time, as a fraction of 8 TB/s.  Needs a GPU; no fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=20, help="log2 lane count")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup-pushes", type=int, default=8)
    ap.add_argument("--settle", type=int, default=400, help="steps run before the steady-state rows")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if pkg.device_count() < 1:
        raise SystemExit("episode_memory_probe: no GPU")
    n = 1 << args.lanes
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    lines, rows = [], {}

    def event_pair():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, before=None, reps=None):
        """Median us of fn() over reps windows; before() runs outside each window (the step a push needs)."""
        ts = []
        for _ in range(reps or args.reps):
            if before:
                before()
            a, b = event_pair()
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return float(np.median(ts)), ts

    with pkg.VectorEnv("CartPole-v1", n, seed=1, auto_reset=True, episode_stats=True, max_episode_steps=500,
                       stream=stream.cuda_stream) as env:
        env.Reset()
        acts = torch.empty(n, dtype=torch.int32, device="cuda")
        tick = [0]

        def sample():
            tick[0] += 1
            env.SampleActionsDevice(acts, seed=3, tick=tick[0])

        def step():
            sample()
            env.StepDevice(acts)

        for _ in range(5):
            step()
        step_us, _ = timed(lambda: env.StepDevice(acts), before=sample)
        mem = env.EpisodeMemory(capacity=100, max_length=500, history=4)
        # warm-up: every ended episode is a candidate until the pool is full
        warm = []
        for _ in range(args.warmup_pushes):
            step()
            before = mem.Stats()["ended"]
            us, _ = timed(lambda: mem.Push(acts), reps=1)
            warm.append((us, mem.Stats()["ended"] - before))
        for _ in range(args.settle):
            step()
            mem.Push(acts)
        env.Sync()
        st0 = mem.Stats()
        steady_us, _ = timed(lambda: mem.Push(acts), before=step)
        st1 = mem.Stats()
        no_done = torch.zeros(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        quiet_us, _ = timed(lambda: mem.Push(acts, no_done), before=step)
        push_bytes = 16 + 4 + 4 + 1 + 8 + 24 + 8
        lines.append(f"lanes 2^{args.lanes} CartPole float32, capacity 100, max_length 500, history 4")
        lines.append(f"step_device                 {step_us:9.2f} us")
        lines.append(f"push, no admission          {quiet_us:9.2f} us  = {quiet_us / step_us:5.2f} x step_device; {push_bytes} B/lane -> "
                     f"{push_bytes * n / (quiet_us * 1e-6) / 1e12:5.2f} TB/s = {push_bytes * n / (quiet_us * 1e-6) / HBM:5.3f} of 8 TB/s")
        lines.append(f"push, steady state          {steady_us:9.2f} us  = {steady_us / step_us:5.2f} x step_device "
                     f"({(st1['admitted'] - st0['admitted']) / args.reps:.1f} admitted per push, kept {st1['kept']})")
        for i, (us, ended) in enumerate(warm):
            lines.append(f"push, warm-up #{i:<2d}          {us:9.2f} us  ({ended} episodes ended)")
        rows.update(step_us=round(step_us, 2), push_quiet_us=round(quiet_us, 2), push_steady_us=round(steady_us, 2),
                    push_bytes_per_lane=push_bytes, warmup=[{"us": round(u, 2), "ended": e} for u, e in warm])
        nrows = mem.DatasetSize()
        lib, h = env._lib, env._h
        x = torch.empty(nrows * 4 * 4, dtype=torch.float32, device="cuda")
        a = torch.empty(nrows, dtype=torch.int32, device="cuda")
        oh = torch.empty(nrows * 2, dtype=torch.float32, device="cuda")
        params_us, _ = timed(lambda: lib.gymnet_vecenv_memory_dataset_device(h, 0, 0, 0, 0, 0, 0, 0, x.data_ptr(), a.data_ptr(),
                                                                              oh.data_ptr(), None, nrows))
        px = torch.empty(nrows * 4 * 800, dtype=torch.float32, device="cuda")
        pix_us, _ = timed(lambda: lib.gymnet_vecenv_memory_dataset_device(h, 4, 200, 150, 200, 150, 40, 20, px.data_ptr(), a.data_ptr(),
                                                                           oh.data_ptr(), None, nrows))
        lines.append(f"dataset build, params       {params_us:9.2f} us  ({nrows} rows of 16 floats)")
        lines.append(f"dataset build, binary_f32   {pix_us:9.2f} us  ({nrows} rows of 4 x 40 x 20 floats)")
        rows.update(dataset_rows=nrows, dataset_params_us=round(params_us, 2), dataset_binary_f32_us=round(pix_us, 2))
    text = "\n".join(lines) + "\n" + json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, **rows}) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
