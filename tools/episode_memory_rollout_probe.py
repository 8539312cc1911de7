"""Times the episode memory's rollout ingest (gymnet_vecenv_memory_push_rollout_device) against the single pushes it replaces, with HIP
events in one process: CartPole float32, 2^20 lanes by default, auto-reset with max_episode_steps 500, capacity 100, max_length 500,
T = 256 steps of random actions from a ring.

    python tools/episode_memory_rollout_probe.py [--lanes 20] [--steps 256] [--chunks 1,4,16,64] [--out profiles/episode_memory_rollout_probe.txt]

Every variant starts from the same checkpoint of the handle and the same action ring, so all of them see the same steps: a warm-up of T
steps that fills the pool, T steps whose memory work alone is timed, and T steps timed as a whole loop.
  (a) single pushes      T x memory_push_device, each after its single step (the steps are outside the timed windows)
  (b) PushRollout, C     one PushRollout of the T rows a fused rollout recorded, memory configured with rollout_chunk C
  (c) whole loop         T x (StepDevice, Push) against mem.Rollout(T, ring): the rollout launch, its recording and the ingest
One run per row, no spread taken.  Needs a GPU; no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=20, help="log2 lane count")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--chunks", default="1,4,16,64")
    ap.add_argument("--settle", type=int, default=64, help="steps run before the checkpoint")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if pkg.device_count() < 1:
        raise SystemExit("episode_memory_rollout_probe: no GPU")
    n, T = 1 << args.lanes, args.steps
    chunks = [int(c) for c in args.chunks.split(",")]
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    lines, rows = [], {}

    def window(fn):
        """us of fn() between two events on the handle's stream"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    with pkg.VectorEnv("CartPole-v1", n, seed=1, auto_reset=True, episode_stats=True, max_episode_steps=500, stream=stream.cuda_stream) as env:
        env.Reset()
        gen = torch.Generator(device="cuda")
        gen.manual_seed(3)
        ring = torch.randint(0, 2, (T, n), dtype=torch.int32, device="cuda", generator=gen)
        torch.cuda.synchronize()
        for t in range(args.settle):
            env.StepDevice(ring[t % T])
        env.Sync()
        ck = env.Checkpoint()
        rec = (torch.empty((T, 4, n), dtype=torch.float32, device="cuda"), torch.empty((T, n), dtype=torch.float32, device="cuda"),
               torch.empty((T, n), dtype=torch.uint8, device="cuda"))

        def fused():
            env.RolloutFusedDevice(ring, T, n, T, rec_obs=rec[0], rec_reward=rec[1], rec_done=rec[2])

        def loop():
            for t in range(T):
                env.StepDevice(ring[t])
                mem.Push(ring[t])

        # (a) and the loop side of (c): the plain config
        env.Restore(ck)
        mem = env.EpisodeMemory(capacity=100, max_length=500, history=4)
        loop()
        env.Sync()
        st0 = mem.Stats()
        push_us = []
        for t in range(T):
            env.StepDevice(ring[t])
            push_us.append(window(lambda: mem.Push(ring[t])))
        st1 = mem.Stats()
        loop_us = window(loop)
        singles = sum(push_us)
        stats = {"single": mem.Stats()}
        lines.append(f"lanes 2^{args.lanes} CartPole float32, capacity 100, max_length 500, T = {T} steps, ring actions; one run, no spread taken")
        lines.append(f"pool after the warm-up: kept {st0['kept']}; the timed {T} steps ended {st1['ended'] - st0['ended']} episodes, admitted "
                     f"{st1['admitted'] - st0['admitted']}")
        lines.append(f"(a) {T} x memory_push_device        {singles:10.1f} us  = {singles / T:7.2f} us per step (median push {sorted(push_us)[T // 2]:.2f} us)")
        rows.update(single_push_total_us=round(singles, 1), single_loop_us=round(loop_us, 1))
        ingest = {}
        for c in chunks:
            env.Restore(ck)
            mem = env.EpisodeMemory(capacity=100, max_length=500, history=4, rollout_chunk=c)
            fused()
            mem.PushRollout(T, rec[0], ring, rec[1], rec[2])
            fused()
            env.Sync()
            us = window(lambda: mem.PushRollout(T, rec[0], ring, rec[1], rec[2]))
            whole = window(lambda: mem.Rollout(T, ring, action_stride=n, ring=T))
            stats[c] = mem.Stats()
            ingest[c] = (us, whole)
            lines.append(f"(b) PushRollout, C = {c:<3d}            {us:10.1f} us  = {us / T:7.2f} us per step  = {singles / us:5.2f} x faster than (a); "
                         f"{2 * -(-T // c)} launches")
        fused()
        env.Sync()
        rollout_us = window(fused)
        lines.append(f"    the fused rollout alone, recording  {rollout_us:8.1f} us  = {rollout_us / T:7.2f} us per step")
        lines.append(f"(c) {T} x (StepDevice, Push)         {loop_us:10.1f} us  = {loop_us / T:7.2f} us per step")
        for c in chunks:
            whole = ingest[c][1]
            lines.append(f"(c) mem.Rollout, C = {c:<3d}            {whole:10.1f} us  = {whole / T:7.2f} us per step  = {loop_us / whole:5.2f} x faster")
        same = all(stats[c] == stats["single"] for c in chunks)
        lines.append(f"every variant ended with the same stats: {same}  {stats['single']}")
        rows.update(push_rollout_us={str(c): round(v[0], 1) for c, v in ingest.items()}, rollout_us={str(c): round(v[1], 1) for c, v in ingest.items()},
                    fused_rollout_recording_us=round(rollout_us, 1), same_stats=same)
    text = "\n".join(lines) + "\n" + json.dumps({"device": torch.cuda.get_device_name(0), "lanes": n, "steps": T, **rows}) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
