"""One handle against a CPU model across mixed call sequences (tests/_call_sequences.py; the model is tests/_handle_replay.py HandleModel,
built from the oracle alone; what the sequences cover is asserted in tests/test_call_sequences_host.py).

What lives BETWEEN launches is what is checked here: the host mirrors of the tick, its slot and the done-count parity, the buffer a
double-buffered handle stands on, the kernel variant the seeds select, and what the captured graphs froze.  After EVERY operation the
handle must equal the model bit for bit (NaN equal to NaN): GetState, Read (observation, reward, done, truncated), the done bytes, Tick
and Counters()["tick"] — the device's own word —, Counters()["lane_steps"], GetSeed and the per-lane keys, steps_beyond_done, the running
and finished episode arrays and terminal observations where kept; after a step-like operation on a done-list handle the sorted
DoneLanes() and DoneRecords(); after a fused rollout every recorded step and the sorted episode records.  A call the table
(_handle_replay.accepted / refusals) accepts and the library refuses, or the reverse, fails.  A failure names the operation's index, the
operation, its entry point and the first differing element; the test id carries the sequence's seed.

The resident configuration (G) is compared in full after every operation its kernel does not serve and after every third one; after the
others by what the call returned and the tick, so that consecutive host steps really are served through the mailbox (every getter but
Tick makes the kernel leave).  Whether those steps were in fact served by the resident kernel is not observable through the API (the
library exposes no served-command or launch counter): residency itself is tests/test_gpu_resident.py's subject, here the resident handle's
host mirrors are."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _call_sequences as Q  # noqa: E402
import _handle_replay as H  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
# what each refused call must raise, and words of its message: a refusal counts only if it is the one that was meant
REFUSALS = {
    "bad_policy": (ValueError, r"launch policy: block = 100"),
    "reset_form1": (ValueError, r"launch policy: reset_form = 1"),
    "misaligned": (ValueError, r"d_actions and action_stride must be \d+-byte aligned"),
    "ring0": (ValueError, r"bad steps/ring/action_stride"),
    "repeat256": (ValueError, r"repeat must be an int in \[0, 255\]"),
    "epsilon": (ValueError, r"epsilon must be in \[0, 1\]"),
    "epsilon:box": (NotImplementedError, r"epsilon-greedy composition is defined for Discrete"),
    "restore_num_envs": (ValueError, r"checkpoint belongs to a different environment / batch size"),
    "set_sbd": (NotImplementedError, r"steps_beyond_done exists only for CartPole without"),
    "set_array": (NotImplementedError, r"array 4 needs GYMNET_FLAG_EPISODE_STATS"),
}
REFUSED = (ValueError, NotImplementedError)


class Driver:
    def __init__(self, pkg, oracle, name):
        import torch
        self.torch, self.pkg, self.name, self.c = torch, pkg, name, H.CONFIGS[name]
        self.n = self.c["n"]
        self.model = H.HandleModel(oracle, self.c)
        self.env = self.open()
        self.bufs, self.slots, self.mslots = {}, {}, {}
        self.stride = (self.n + 3) // 4 * 4         # whole lane groups of every width: a rollout's slices stay aligned
        self.box = H.M.ENVS[self.c["env"]]["box"]
        self.i, self.op = -1, None

    def open(self):
        c = self.c
        kw = dict(seed=H.SEED, auto_reset=c["auto_reset"], dtype=np.float64 if c["f64"] else np.float32, lane_offset=c["lane_offset"],
                  done_list=c["done_list"], episode_stats=c["episode_stats"], final_obs=c["final_obs"], max_episode_steps=c["max_episode_steps"],
                  double_buffer=c["double_buffer"], resident=c["resident"])
        if c["launch"]:
            kw["launch_policy"] = c["launch"]
        return self.pkg.VectorEnv(c["gym"], c["n"], **kw)

    def close(self):
        self.env.Close()

    # -- helpers -----------------------------------------------------------------------------------------------------------------
    def where(self):
        op = self.op
        what = op.get("path") or op.get("what") or op.get("name") or ""
        return f"config {self.name}, op {self.i}: {op['kind']} {what}"

    def same(self, label, got, want):
        d = H.first_diff(got, want)
        assert d is None, f"{self.where()}: {label} differs at {d[0]}: handle {d[1]!r}, model {d[2]!r}"

    def device(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.torch.cuda.synchronize()
        return t

    def buf(self, op):
        """the persistent action buffer an operation names: the same pointer, stride and ring at every use"""
        R = len(op["ring"])
        if op["buf"] not in self.bufs:
            self.bufs[op["buf"]] = self.torch.zeros((R, self.stride), dtype=self.torch.float32 if self.box else self.torch.int32, device="cuda")
        b = self.bufs[op["buf"]]
        if op["fill"]:
            self.env.Sync()
            b[:, :self.n] = self.torch.from_numpy(np.ascontiguousarray(op["ring"]))
        self.torch.cuda.synchronize()
        return b

    def returned(self, obs=None, reward=None, done=None, truncated=None):
        m = self.model
        if obs is not None:
            self.same("returned observation", np.asarray(obs).T, m.obs)
        if reward is not None:
            self.same("returned reward", reward, m.reward)
        if done is not None:
            self.same("returned done", np.asarray(done).astype(bool), m.done != 0)
        if truncated is not None:
            self.same("returned truncated", truncated, (m.done & 2) != 0)

    # -- one operation on the handle; returns what the call handed back, to be compared once the model has taken the operation too --
    def call(self, op):
        env, n, k, torch = self.env, self.n, op["kind"], self.torch
        if k == "step":
            a, p = op["a"], op["path"]
            if p in ("Step", "StepInt"):
                out = env.Step(int(a) if p == "StepInt" else a)
            elif p == "StepInto":
                pa, po, pr, pd = env.HostBuffers()
                pa[:] = a
                env.StepInto(pa, po, pr, pd)
                return dict(obs=po.copy(), reward=pr.copy(), done=pd.copy(), truncated=(pd & 2) != 0)
            elif p == "StepAsync":
                out = env.StepAsync(a).Result()
            else:
                self.keep = self.device(a)
                env.StepDevice(self.keep)
                return {}
            return dict(obs=out.Observation, reward=out.Reward, done=out.Done, truncated=out.Truncated)
        if k == "rollout" and op["path"] != "fused":
            b = self.buf(op)
            env.SetLaunchPolicy(graph=1 if op["path"] == "graph" else 0)
            env.RolloutDevice(b, op["T"], self.stride, len(op["ring"]))
            return {}
        if k in ("rollout", "rollout_sampled", "rollout_eps"):
            T, O = op["T"], H.obs_dim(self.c)
            rec = dict(rec_obs=torch.zeros((T, O, n), dtype=torch.float64 if self.c["f64"] else torch.float32, device="cuda"),
                       rec_reward=torch.zeros((T, n), dtype=torch.float32, device="cuda"), rec_done=torch.zeros((T, n), dtype=torch.uint8, device="cuda"))
            ep = None
            if k != "rollout":
                rec["rec_actions"] = torch.zeros((T, n), dtype=torch.float32 if self.box else torch.int32, device="cuda")
            if self.c["episode_stats"]:
                cap = n * T
                ep = dict(step=torch.full((cap,), -1, dtype=torch.int32, device="cuda"), lane=torch.full((cap,), -1, dtype=torch.int32, device="cuda"),
                          ret=torch.zeros(cap, dtype=torch.float32, device="cuda"), length=torch.zeros(cap, dtype=torch.int32, device="cuda"),
                          capacity=cap, count=torch.zeros(2, dtype=torch.uint32, device="cuda"))
            if k == "rollout_sampled":
                torch.cuda.synchronize()
                env.RolloutFusedDevice(None, T, actions="sample", action_seed=op["aseed"], action_tick0=op["atick0"], episodes=ep, **rec)
            else:
                b = self.buf(op)
                more = dict(actions="epsilon_greedy", action_seed=op["aseed"], action_tick0=op["atick0"], epsilon=op["eps"]) if k == "rollout_eps" else {}
                env.RolloutFusedDevice(b, T, self.stride, len(op["ring"]), episodes=ep, **rec, **more)
            env.Sync()
            return dict(fused=rec, episodes=ep)
        if k == "decision":
            if op["path"] == "StepRepeat":
                out = env.StepRepeat(op["a"], op["R"] - 1)
                return dict(obs=out.Observation, reward=out.Reward, done=out.Done, truncated=out.Truncated)
            self.keep = self.device(op["a"])
            env.StepRepeatDevice(self.keep, op["R"] - 1)
            return {}
        if k == "reset":
            return dict(obs=env.Reset()) if op["path"] == "Reset" else (env.ResetDevice() or {})
        if k == "reset_where":
            if op["path"] == "ResetWhere":
                return dict(obs=env.ResetWhere(op["mask"]))
            self.keep = None if op["mask"] is None else self.device(op["mask"])
            env.ResetWhereDevice(self.keep)
            return {}
        if k == "seed":
            env.Seed(op["value"])
        elif k == "set_lane_seeds":
            env.SetArray("lane_seeds", np.asarray(op["value"]).astype(np.uint64))
        elif k == "set_tick":
            env.Tick = op["value"]
        elif k == "set_state":
            env.SetState(op["state"])
        elif k == "set_array":
            env.SetArray(op["name"], op["value"])
        elif k == "set_sbd":
            env.SetStepsBeyondDone(op["value"])
        elif k == "checkpoint":
            self.slots[op["slot"]] = env.Checkpoint()
        elif k == "restore":
            env.Restore(self.slots[op["slot"]])
        elif k == "migrate":                        # a fresh handle of the same arguments continues in this one's place
            ck, pol = env.Checkpoint(), env.GetLaunchPolicy()
            new = self.open()
            new.SetLaunchPolicy(**{f: pol[f] for f in ("vec", "block", "nt", "reset_form", "graph")})
            new.Restore(ck)
            env.Close()
            self.env = new
        elif k == "noop":
            w = op["what"]
            if w == "policy":
                env.SetLaunchPolicy(**op["fields"])
            elif w == "Sync":
                env.Sync()
            elif w == "GetState":
                env.GetState()
            elif w == "KernelName":
                assert env.KernelName()
            else:
                t = torch.zeros((n, H.obs_dim(self.c)), dtype=torch.float64 if self.c["f64"] else torch.float32, device="cuda")
                torch.cuda.synchronize()
                env.PackObsDevice(t)
                env.Sync()
                return dict(obs=t.cpu().numpy())
        return {}

    def refused(self, op):
        env, n, w = self.env, self.n, op["what"]
        if w == "bad_policy":
            env.SetLaunchPolicy(block=100)
        elif w == "reset_form1":
            env.SetLaunchPolicy(reset_form=1)
        elif w == "misaligned":
            assert n % self.c["wide"] != 0 and env.GetLaunchPolicy()["vec"] == self.c["wide"]
            env.RolloutDevice(self.buf(op), 3, n, 3)
        elif w == "ring0":
            env.RolloutDevice(self.buf(op), 3, self.stride, 0)
        elif w == "repeat256":
            env.StepRepeat(op["a"], 256)
        elif w == "epsilon":
            env.RolloutFusedDevice(self.buf(op), 3, self.stride, 3, actions="epsilon_greedy", epsilon=1.5)
        elif w == "restore_num_envs":
            env.Restore(dict(env.Checkpoint(), num_envs=n + 1))
        elif w == "set_sbd":
            env.SetStepsBeyondDone(op["value"])
        elif w == "set_array":
            env.SetArray("episode_length", op["value"])
        else:
            raise KeyError(w)

    # -- the comparison ------------------------------------------------------------------------------------------------------------
    def compare(self, full):
        env, m, c = self.env, self.model, self.c
        assert env.Tick == m.tick, f"{self.where()}: Tick {env.Tick}, model {m.tick}"
        if not full:
            return
        self.same("GetState", env.GetState(), m.s)
        r = env.Read()
        self.returned(r.Observation, r.Reward, r.Done, r.Truncated)
        self.same("done bytes", env.GetArray("done"), m.done)
        self.same("reward array", env.GetArray("reward"), m.reward)
        cnt = env.Counters()
        assert cnt["tick"] == m.tick, f"{self.where()}: the device's tick word {cnt['tick']}, model {m.tick} (host mirror {env.Tick})"
        assert cnt["lane_steps"] == m.lane_steps, f"{self.where()}: lane_steps {cnt['lane_steps']}, model {m.lane_steps}"
        assert env.GetSeed() == (m.seed, m.seeds is not None), f"{self.where()}: GetSeed {env.GetSeed()}, model {(m.seed, m.seeds is not None)}"
        if m.seeds is not None:
            self.same("lane_seeds", env.GetArray("lane_seeds"), m.seeds)
        if m.sbd is not None:
            self.same("steps_beyond_done", env.GetStepsBeyondDone(), m.sbd)
        if c["episode_stats"]:
            for name, want in (("episode_return", m.ret), ("episode_length", m.ln), ("finished_return", m.fin_ret), ("finished_length", m.fin_len)):
                self.same(name, env.GetArray(name), want)
        if c["final_obs"]:
            self.same("final_obs", env.GetArray("final_obs"), m.final)

    def compare_done_list(self):
        env, m, c = self.env, self.model, self.c
        fin = m.last_fin
        self.same("DoneLanes", np.sort(env.DoneLanes()), np.nonzero(fin)[0].astype(np.int32))
        rec = env.DoneRecords()
        order = np.argsort(rec["lanes"])
        self.same("DoneRecords lanes", rec["lanes"][order], np.nonzero(fin)[0].astype(np.int32))
        if c["episode_stats"]:
            self.same("DoneRecords return", rec["return"][order], m.fin_ret[fin])
            self.same("DoneRecords length", rec["length"][order], m.fin_len[fin])
        if c["final_obs"]:
            self.same("DoneRecords final_obs", rec["final_obs"][order], m.final[:, fin].T)

    def compare_fused(self, got, recs):
        rec, ep = got["fused"], got["episodes"]
        o, rw, dn = rec["rec_obs"].cpu().numpy(), rec["rec_reward"].cpu().numpy(), rec["rec_done"].cpu().numpy()
        act = rec["rec_actions"].cpu().numpy() if "rec_actions" in rec else None
        for t, want in enumerate(recs):
            if act is not None:
                self.same(f"recorded action, step {t}", act[t], want["a"])
            self.same(f"recorded observation, step {t}", o[t], want["obs"])
            self.same(f"recorded reward, step {t}", rw[t], want["reward"])
            self.same(f"recorded done, step {t}", dn[t], want["done"])
        if ep is not None:
            cnt = ep["count"].cpu().numpy().astype(np.int64)
            k = int(cnt[0])
            got_rec = np.stack([ep["step"].cpu().numpy()[:k], ep["lane"].cpu().numpy()[:k], ep["length"].cpu().numpy()[:k]], axis=1)
            got_ret = ep["ret"].cpu().numpy()[:k]
            order = np.lexsort((got_rec[:, 1], got_rec[:, 0]))
            want = np.concatenate([np.stack([np.full(len(r["lanes"]), t), r["lanes"], r["fin_len"]], axis=1) for t, r in enumerate(recs)])
            assert cnt[0] == cnt[1] == len(want), f"{self.where()}: episode records {cnt}, model {len(want)}"
            self.same("episode records (step, lane, length)", got_rec[order], want)
            self.same("episode records' returns", got_ret[order], np.concatenate([r["fin_ret"] for r in recs]))

    # -- one operation, both sides -----------------------------------------------------------------------------------------------
    def run(self, i, op):
        self.i, self.op = i, op
        k = op["kind"]
        if k == "refused":
            exc, words = REFUSALS[op["what"] + (":box" if op["what"] == "epsilon" and self.box else "")]
            with pytest.raises(exc, match=words):
                self.refused(op)
                pytest.fail(f"{self.where()}: the library accepted a call the table refuses")
            got = {}
        else:
            try:
                got = self.call(op)
            except REFUSED as e:
                pytest.fail(f"{self.where()}: the library refused a call the table accepts: {e!r}")
        recs = H.apply(self.model, op, self.mslots)
        self.returned(got.get("obs"), got.get("reward"), got.get("done"), got.get("truncated"))
        served = (k == "step" and op["path"] in ("Step", "StepInt", "StepInto")) or (k == "reset" and op["path"] == "Reset")
        full = not self.c["resident"] or not served or i % 3 == 2
        self.compare(full)
        if "fused" in got:
            self.compare_fused(got, recs)
        if full and k in H.STEP_LIKE and self.c["done_list"]:
            self.compare_done_list()


def _run(gpu_pkg, oracle, name, ops):
    d = Driver(gpu_pkg, oracle, name)
    try:
        for i, op in enumerate(ops):
            d.run(i, op)
    finally:
        d.close()


@pytest.mark.parametrize("seed", Q.MIXED_SEEDS)
@pytest.mark.parametrize("name", sorted(H.CONFIGS))
def test_a_mixed_sequence_leaves_the_handle_equal_to_the_model_after_every_operation(gpu_pkg, oracle, name, seed):
    _run(gpu_pkg, oracle, name, Q.mixed(name, seed))


@pytest.mark.parametrize("name", sorted(H.CONFIGS))
def test_every_row_of_the_table_is_held_to_the_library(gpu_pkg, oracle, name):
    """Scripted, nothing drawn: every refusal the table lists for the configuration (by exception type and message), every launch-policy
    form it accepts, Sync / GetState / KernelName / PackObsDevice, Seed(int) / Seed(keys) / Seed(equal keys), ResetWhere(None) through
    both entry points — each followed by a compared step."""
    _run(gpu_pkg, oracle, name, Q.table(name))


@pytest.mark.parametrize("name, mutator", [(n, m) for n in sorted(Q.STALE) for m in Q.STALE[n]])
def test_a_warm_graph_cache_survives_the_mutator(gpu_pkg, oracle, name, mutator):
    """Eight captured graphs — both action buffers at every parity combination — then one mutator, then the same rollouts again: a graph
    that kept the old seed, keys, configuration or buffers would replay and the handle would leave the model."""
    ops, _ = Q.stale_graph(name, mutator)
    _run(gpu_pkg, oracle, name, ops)
