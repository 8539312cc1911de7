"""Times what recording a Box actor's log-density and a critic's value costs a fused actor rollout (gym.net_amd/csrc/actor_box_logd.hip),
with HIP events in one process: Pendulum with an actor [12, 50, 20, 1] and a critic [12, 50, 20, 1], MountainCarContinuous with
[8, 50, 20, 1] twice (history 4), float32, 2^20 lanes by default, auto-reset, epsilon 1 under ("tanh", "gaussian", 0.3) — every lane draws
its noise.

    python tools/actor_box_logd_probe.py [--lanes 20] [--reps 7] [--steps 256] [--passes 2] [--out profiles/actor_box_logd_probe.txt]

Rows per env (us per vector step, median of --reps timings, at least five):
  a  rec_actions              one GYMNET_ACTIONS_ACTOR rollout of --steps steps recording the actions: actor_box_policy.hip's kernel
  b  + rec_logd               the same rollout also recording rec_logd: actor_box_logd.hip's kernel
  c  + rec_value              (b) also recording rec_value: the same kernel, the critic's forward pass inside it
  d  rec_obs + torch          what a caller did before rec_logd: the rollout of (a) also recording rec_obs and rec_done, then the recorded
                              inputs through torch — the history of every step rebuilt across episode ends, actor and critic as three addmm
                              each, the tanh head and Normal(g, sigma).log_prob(rec_actions); the rollout part and the torch part are also
                              given apart
  v  Value()                  the stand-alone value kernel, one launch over the current history (us per call: it is one vector step's worth)
The variants alternate on the same handle, twice; the second round is the one kept.  The whole measurement runs --passes times (a fresh
handle each), so a run-to-run spread exists: the table gives each pass and, per row, the spread between the passes.  Needs a GPU; no
fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENVS = [("Pendulum-v1", 3, -2.0, 2.0), ("MountainCarContinuous-v0", 2, -1.0, 1.0)]
HISTORY, EPS = 4, 1.0
POLICY = ("tanh", "gaussian", 0.3)
CHUNK = 32                                             # steps per torch pass of (d): bounds its working set at 2^20 lanes


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
        raise SystemExit("actor_box_logd_probe: no GPU")
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

    def mlp(win):
        return torch.nn.Sequential(torch.nn.Linear(win, 50), torch.nn.ReLU(), torch.nn.Linear(50, 20), torch.nn.ReLU(), torch.nn.Linear(20, 1)).cuda()

    lines = [f"lanes 2^{args.lanes} float32 auto-reset, actor and critic [{HISTORY} * obs_dim, 50, 20, 1] (history {HISTORY}), {POLICY}, epsilon {EPS}, "
             f"fused T = {T}, median of {reps}; us per vector step; {args.passes} passes"]
    rows = {}
    for p in range(args.passes):
        for name, O, low, high in ENVS:
            torch.manual_seed(0)
            seq, critic = mlp(HISTORY * O), mlp(HISTORY * O)
            mid, half = 0.5 * (low + high), 0.5 * (high - low)
            with pkg.VectorEnv(name, n, seed=1, auto_reset=True, stream=stream.cuda_stream) as env:
                env.Reset()
                actor = env.Actor(seq, history=HISTORY)
                actor.SetCritic(critic)
                actor.SetPolicy(*POLICY)
                for t in range(5):
                    actor.Step(EPS, 7, t)
                rec_act = torch.empty((T, n), dtype=torch.float32, device="cuda")
                rec_logd = torch.empty((T, n), dtype=torch.float32, device="cuda")
                rec_value = torch.empty((T, n), dtype=torch.float32, device="cuda")
                rec_obs = torch.empty((T, O, n), dtype=torch.float32, device="cuda")
                rec_done = torch.empty((T, n), dtype=torch.uint8, device="cuda")
                hist = torch.empty((n, HISTORY, O), dtype=torch.float32, device="cuda")
                out_v = torch.empty((T, n), dtype=torch.float32, device="cuda")
                out_l = torch.empty((T, n), dtype=torch.float32, device="cuda")
                last = torch.empty(n, dtype=torch.float32, device="cuda")
                kw = dict(actions="actor", epsilon=EPS, action_seed=7, action_tick0=0, rec_actions=rec_act)

                def rollout_a():
                    env.RolloutFusedDevice(None, T, **kw)

                def rollout_b():
                    env.RolloutFusedDevice(None, T, rec_logd=rec_logd, **kw)

                def rollout_c():
                    env.RolloutFusedDevice(None, T, rec_logd=rec_logd, rec_value=rec_value, **kw)

                def rollout_d():
                    env.RolloutFusedDevice(None, T, rec_obs=rec_obs, rec_done=rec_done, **kw)

                def torch_d():
                    # the inputs of step t are the history BEFORE it: rebuilt from the recorded observations and done bytes as the actor's
                    # push keeps it (a lane that ended refills every slot).  The history the rollout started from would be needed for
                    # exact numbers; the probe times the work, so it starts from the first recorded observation
                    with torch.no_grad():
                        hist.copy_(rec_obs[0].t()[:, None, :].expand(n, HISTORY, O))
                        for t0 in range(0, T, CHUNK):
                            xs = []
                            for t in range(t0, min(T, t0 + CHUNK)):
                                xs.append(hist.reshape(n, HISTORY * O).clone())
                                o = rec_obs[t].t()
                                rolled = torch.cat([hist[:, 1:], o[:, None, :]], dim=1)
                                hist.copy_(torch.where((rec_done[t] != 0)[:, None, None], o[:, None, :].expand(n, HISTORY, O), rolled))
                            x = torch.stack(xs)
                            out_v[t0:t0 + len(xs)] = critic(x)[..., 0]
                            g = mid + half * torch.tanh(seq(x)[..., 0])
                            out_l[t0:t0 + len(xs)] = torch.distributions.Normal(g, POLICY[2]).log_prob(rec_act[t0:t0 + len(xs)])

                def both_d():
                    rollout_d()
                    torch_d()

                def value_v():
                    actor.Value(out=last)
                for _ in range(2):                                   # each variant twice, alternating: the second round is the one kept
                    r = {"a_us": timed(rollout_a) / T, "b_us": timed(rollout_b) / T, "c_us": timed(rollout_c) / T, "d_rollout_us": timed(rollout_d) / T}
                    r["d_torch_us"] = timed(torch_d) / T
                    r["d_us"] = timed(both_d) / T
                    r["v_us"] = timed(value_v)
                rows.setdefault(name, [None] * args.passes)[p] = {k: round(v, 2) for k, v in r.items()}
    for name, _, _, _ in ENVS:
        for p, r in enumerate(rows[name]):
            lines.append(f"{name:24s} pass {p + 1}   a rec_actions {r['a_us']:8.2f} us   b + rec_logd {r['b_us']:8.2f} us   c + rec_value {r['c_us']:8.2f} us   "
                         f"d rec_obs + torch {r['d_us']:8.2f} us (rollout {r['d_rollout_us']:.2f} + torch {r['d_torch_us']:.2f})   v Value() {r['v_us']:8.2f} us")
        a, b, c, d, v = (np.array([r[k] for r in rows[name]]) for k in ("a_us", "b_us", "c_us", "d_us", "v_us"))
        lines.append(f"{name:24s} b - a per pass: " + ", ".join(f"{x:+.2f} us" for x in b - a) + "   c - b per pass: " + ", ".join(f"{x:+.2f} us" for x in c - b) +
                     "   beside Value(): " + ", ".join(f"{x:.2f} us" for x in v) + "   c < d per pass: " + ", ".join(str(bool(x < y)) for x, y in zip(c, d)) +
                     f"   spread between passes: a {a.max() - a.min():.2f} us, b {b.max() - b.min():.2f} us, c {c.max() - c.min():.2f} us, "
                     f"d {d.max() - d.min():.2f} us, v {v.max() - v.min():.2f} us")
    text = "\n".join(lines) + "\n" + json.dumps({"device": torch.cuda.get_device_name(0), "reps": reps, "lanes": n, "steps": T, "epsilon": EPS,
                                                 "policy": list(POLICY), "passes": args.passes, "rows": rows}) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
