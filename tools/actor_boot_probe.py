"""Times what recording V(terminal observation) on time-limit rows costs a fused actor rollout (gym.net_amd/csrc/actor_boot.hip), with HIP
events in one process, float32, 2^20 lanes by default, auto-reset, history 4, epsilon 1:
  CartPole   actor [16, 50, 20, 2] under ("softmax", 1.0), critic [16, 50, 20, 1], max_episode_steps 500, the running episode lengths
             staggered over [0, 500) as a long-running handle has them (SetArray, put back in front of every timed launch: a random policy
             drops the pole within some twenty steps, so only the lanes that close to the limit reach it)
  Pendulum   actor and critic [12, 50, 20, 1] under ("tanh", "gaussian", 0.3), max_episode_steps 200, all lanes synchronous: the worst case,
             every wave pays in the same step

    python tools/actor_boot_probe.py [--lanes 20] [--reps 7] [--steps 256] [--passes 2] [--out profiles/actor_boot_probe.txt]

Rows per env (us per vector step, median of --reps timings, at least five):
  a  rec_value          one GYMNET_ACTIONS_ACTOR rollout of --steps steps recording actions, logp / logd, done bytes and values: the parent's
                        kernel (actor_value.hip / actor_box_logd.hip)
  b  + rec_boot         the same rollout also recording rec_boot: actor_boot.hip's kernel
  c  single steps       what a caller did before rec_boot to get the same array: --steps x (Act with the value, StepDevice, the dense final
                        observations and done bytes read on the device, the critic through torch on the rebuilt input, Push)
  v  Value()            the stand-alone value kernel (us per call: one vector step's worth)
and the share of (wave, step) pairs of (b)'s rollout in which a wave holds a truncated lane, from its rec_done: v times that share is the
cost the ballot skip predicts for b - a, beside one 4-byte store per lane-step.  The variants alternate on the same handle, twice; the
second round is the one kept.  The whole measurement runs --passes times (a fresh handle each): the table gives each pass and, per row,
the spread between the passes.  Needs a GPU; no fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENVS = [("CartPole-v1", 4, 2, 500, False), ("Pendulum-v1", 3, 1, 200, True)]         # name, obs_dim, last width, limit, box
HISTORY, EPS = 4, 1.0
SETTING, POLICY = ("softmax", 1.0), ("tanh", "gaussian", 0.3)


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
        raise SystemExit("actor_boot_probe: no GPU")
    n, T = 1 << args.lanes, args.steps
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)

    def timed(fn, prep=None):
        ts = []
        for _ in range(reps):
            if prep:
                prep()                                               # outside the timed region
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return float(np.median(ts))

    def mlp(win, wout):
        return torch.nn.Sequential(torch.nn.Linear(win, 50), torch.nn.ReLU(), torch.nn.Linear(50, 20), torch.nn.ReLU(), torch.nn.Linear(20, wout)).cuda()

    def device_array(ptr, shape, typestr):
        class _View:                            # the library's buffer, seen by torch without a copy
            __cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}
        return torch.as_tensor(_View(), device="cuda")

    lines = [f"lanes 2^{args.lanes} float32 auto-reset, history {HISTORY}, actor / critic [{HISTORY} * obs_dim, 50, 20, A / 1], epsilon {EPS}, fused T = {T}, "
             f"median of {reps}; us per vector step; {args.passes} passes"]
    rows = {}
    for p in range(args.passes):
        for name, O, A, limit, box in ENVS:
            torch.manual_seed(0)
            seq, critic = mlp(HISTORY * O, A), mlp(HISTORY * O, 1)
            with pkg.VectorEnv(name, n, seed=1, auto_reset=True, episode_stats=True, max_episode_steps=limit, final_obs=True,
                               stream=stream.cuda_stream) as env:
                env.Reset()
                actor = env.Actor(seq, history=HISTORY)
                actor.SetCritic(critic)
                if box:
                    actor.SetPolicy(*POLICY)
                else:
                    actor.SetExploration(*SETTING)
                stagger = None if box else (np.arange(n, dtype=np.int64) * 2654435761 % limit).astype(np.int32)     # over [0, limit)

                def prep():
                    # a random policy drops the pole within some twenty steps and the lane's length starts again at 0, so the staggering
                    # is put back in front of every timed launch: the lanes that are within that many steps of the limit reach it
                    if stagger is not None:
                        env.SetArray("episode_length", stagger)
                        env.Sync()
                for t in range(5):
                    actor.Step(EPS, 7, t)
                view = env.DeviceView()
                final_obs = device_array(view.d_final_obs, (O, n), "<f4")
                done_now = device_array(view.d_done, (n,), "|u1")
                rec_act = torch.empty((T, n), dtype=torch.float32 if box else torch.int32, device="cuda")
                rec_lp, rec_value, rec_boot = (torch.empty((T, n), dtype=torch.float32, device="cuda") for _ in range(3))
                rec_done = torch.empty((T, n), dtype=torch.uint8, device="cuda")
                hist = torch.zeros((n, HISTORY, O), dtype=torch.float32, device="cuda")
                lp, val, last = (torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(3))
                obs_rm = torch.empty((n, O), dtype=torch.float32, device="cuda")
                kw = dict(actions="actor", epsilon=EPS, action_seed=7, action_tick0=0, rec_actions=rec_act, rec_done=rec_done, rec_value=rec_value)
                kw.update(rec_logd=rec_lp) if box else kw.update(rec_logp=rec_lp)

                def rollout_a():
                    env.RolloutFusedDevice(None, T, **kw)

                def rollout_b():
                    env.RolloutFusedDevice(None, T, rec_boot=rec_boot, **kw)

                def steps_c():
                    # the caller's own history stands in for the actor's ring (rebuilt as the push keeps it); exact numbers would need the
                    # ring the loop started from: the probe times the work
                    with torch.no_grad():
                        for t in range(T):
                            if box:
                                actor.Value(out=val)
                                acts = actor.Act(EPS, 7, t, logd=lp)
                            else:
                                acts = actor.Act(EPS, 7, t, logp=lp, value=val)
                            env.StepDevice(acts)
                            x = torch.cat([hist[:, 1:].reshape(n, -1), final_obs.t()], dim=1)
                            rec_boot[t] = torch.where((done_now & 2) != 0, critic(x)[:, 0], torch.zeros((), device="cuda"))
                            env.PackObsDevice(obs_rm)
                            rolled = torch.cat([hist[:, 1:], obs_rm[:, None, :]], dim=1)
                            hist.copy_(torch.where((done_now != 0)[:, None, None], obs_rm[:, None, :].expand(n, HISTORY, O), rolled))
                            actor.Push()

                def value_v():
                    actor.Value(out=last)
                for _ in range(2):                                   # each variant twice, alternating: the second round is the one kept
                    r = {"a_us": timed(rollout_a, prep) / T}
                    r["b_us"] = timed(rollout_b, prep) / T
                    env.Sync()
                    d = (rec_done & 2) != 0
                    pad = (-n) % 64
                    waves = torch.nn.functional.pad(d, (0, pad)).reshape(T, -1, 64).any(dim=2)
                    r["share"] = float(waves.float().mean().item())
                    r["truncated_rows"] = int(d.sum().item())
                    r["c_us"] = timed(steps_c, prep) / T
                    r["v_us"] = timed(value_v)
                rows.setdefault(name, [None] * args.passes)[p] = {k: (round(v, 2) if k.endswith("_us") else v) for k, v in r.items()}
    for name, *_ in ENVS:
        for p, r in enumerate(rows[name]):
            lines.append(f"{name:14s} pass {p + 1}   a rec_value {r['a_us']:8.2f} us   b + rec_boot {r['b_us']:8.2f} us   c single steps + torch {r['c_us']:8.2f} us   "
                         f"v Value() {r['v_us']:8.2f} us   waves with a truncated lane {r['share']:.5f} of (wave, step) pairs, {r['truncated_rows']} truncated rows")
        a = np.array([r["a_us"] for r in rows[name]])
        b = np.array([r["b_us"] for r in rows[name]])
        c = np.array([r["c_us"] for r in rows[name]])
        v = np.array([r["v_us"] for r in rows[name]])
        share = np.array([r["share"] for r in rows[name]])
        lines.append(f"{name:14s} b - a per pass: " + ", ".join(f"{x:+.2f} us" for x in b - a) + "   the ballot skip predicts v * share: " +
                     ", ".join(f"{x:.2f} us" for x in v * share) + "   b < c per pass: " + ", ".join(str(bool(x < y)) for x, y in zip(b, c)) +
                     f"   spread between passes: a {a.max() - a.min():.2f} us, b {b.max() - b.min():.2f} us, c {c.max() - c.min():.2f} us, v {v.max() - v.min():.2f} us")
    text = "\n".join(lines) + "\n" + json.dumps({"device": torch.cuda.get_device_name(0), "reps": reps, "lanes": n, "steps": T, "epsilon": EPS,
                                                 "passes": args.passes, "rows": rows}) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
