"""SQ counters of the actor's kernels (gym.net_amd/csrc/actor.hip) at 2^20 CartPole lanes with the Parameters runner's 16-50-20-2 net:
instructions per env-step by kind, and where the waves' cycles go.  Two parts, because counters are collected in a run of their own:

    rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SMEM SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU \\
        -d OUT -o pmc -- python tools/actor_pmc.py run
    python tools/actor_pmc.py parse OUT [--out profiles/actor_pmc.txt]

run: 4 act launches, then 2 fused actor rollouts of 64 steps (plain auto-reset handle).  parse: per kernel, averaged over its dispatches:
VALU / SMEM instructions per env-step, SQ_ACTIVE_INST_VALU / SQ_WAVE_CYCLES (the share of a wave's life spent issuing VALU),
SQ_WAIT_ANY / SQ_WAVE_CYCLES (waiting on a counter: s_waitcnt for memory or scalar loads) and SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES
(ready but not issued)."""
import argparse
import glob
import json
import os
import re
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, T = 1 << 20, 64


def run():
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    torch.manual_seed(0)
    seq = torch.nn.Sequential(torch.nn.Linear(16, 50), torch.nn.ReLU(), torch.nn.Linear(50, 20), torch.nn.ReLU(), torch.nn.Linear(20, 2))
    with pkg.VectorEnv("CartPole-v1", N, seed=1, auto_reset=True) as env:
        env.Reset()
        actor = env.Actor(seq, history=4)
        out = torch.empty(N, dtype=torch.int32, device="cuda")
        for k in range(4):
            actor.Act(0.1, 7, k, out=out)
        for k in range(2):
            env.RolloutFusedDevice(None, T, actions="actor", epsilon=0.1, action_seed=7, action_tick0=64 * k)
        env.Sync()


def parse(d, out):
    lines = [f"# tools/actor_pmc.py: SQ counters, 2^20 CartPole lanes, 16-50-20-2, averaged over each kernel's dispatches"]
    res = {}
    for db in glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True):
        c = sqlite3.connect(db)
        rows = c.execute("select kernel_name, counter_name, count(*), avg(value), avg(duration) from counters_collection "
                         "where kernel_name like '%actor_%' group by kernel_name, counter_name").fetchall()
        for k, cn, cnt, avg, dur in rows:
            name = re.sub(r"\(.*$", "", k).replace("gymnet::", "").replace("void ", "")
            res.setdefault(name, {})[cn] = avg
            res[name]["_dur_us"] = dur / 1e3
            res[name]["_n"] = cnt
    for name, v in sorted(res.items()):
        steps = T if name.startswith("actor_rollout_kernel") else 1
        env_steps = N * steps
        waves = v.get("SQ_WAVES", 0) or 1
        wc = v.get("SQ_WAVE_CYCLES", 0) or 1
        row = {"dispatches": v["_n"], "us_per_dispatch_under_pmc": round(v["_dur_us"], 1),
               "valu_per_env_step": round(v.get("SQ_INSTS_VALU", 0) * 64 / env_steps, 1),     # per-wave instructions x 64 lanes / env-steps
               "smem_per_env_step": round(v.get("SQ_INSTS_SMEM", 0) * 64 / env_steps, 2),
               "valu_active_share": round(v.get("SQ_ACTIVE_INST_VALU", 0) / wc, 3),
               "wait_any_share": round(v.get("SQ_WAIT_ANY", 0) / wc, 3),
               "wait_inst_any_share": round(v.get("SQ_WAIT_INST_ANY", 0) / wc, 3),
               "waves": int(waves)}
        lines.append(f"{name}: " + json.dumps(row))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("run", "parse"))
    ap.add_argument("dir", nargs="?")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    run() if a.mode == "run" else parse(a.dir, a.out)
