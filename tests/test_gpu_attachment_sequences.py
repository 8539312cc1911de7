"""One handle WITH its attachments against the CPU model across call sequences (tests/_attachment_sequences.py; the model is
tests/_attachment_replay.py AttachedModel on tests/_handle_replay.py HandleModel; what the sequences cover is asserted in
tests/test_attachment_sequences_host.py).

After EVERY operation the handle equals the model in everything tests/test_gpu_call_sequences.py compares, and: actor.History() and the
ring slot; the pixel stack's slots; the memory's counters and kept episodes (the params dataset every 8th operation and at the end).  Act's
actions, logits, log-probabilities and values, Value(), Boot() and the fused actor rollout's recorded steps are compared with the C twins
over the model's history: twin.same for logits, values and boots, raw bits for everything else.  A call the model's staleness state
refuses must raise ValueError (GYMNET_ERR_INVALID_ARG) with the unit's message, and leave everything above equal to the unchanged model.
The gray frame the stack's model is fed comes from RenderDevice on the handle under test (see tests/_attachment_replay.py)."""
import numpy as np
import pytest

import _actor_twin as twin
import _attachment_replay as A
import _attachment_sequences as AQ
import _handle_replay as H
import test_gpu_call_sequences as base

pytestmark = pytest.mark.gpu
PAD, TAIL, SENTINEL = 12, 64, -12345.5


class Driver(base.Driver):
    def __init__(self, pkg, oracle, name):
        import torch
        self.torch, self.pkg, self.name, self.c = torch, pkg, name, A.CONFIGS[name]
        self.n = self.c["n"]
        self.model = A.AttachedModel(oracle, self.c)
        self.ext = []
        self.O, self.A = H.obs_dim(self.c), A.outputs_of(self.c)
        self.box = self.c["box"]
        self.adtype = np.float32 if self.box else np.int32
        self.env = self.open()
        self.bufs, self.slots, self.mslots = {}, {}, {}
        self.stride = (self.n + 3) // 4 * 4
        self.i, self.op = -1, None
        self.actor = self.stack = self.memory = None

    def open(self):
        c, torch = self.c, self.torch
        kw = dict(seed=H.SEED, auto_reset=c["auto_reset"], dtype=np.float64 if c["f64"] else np.float32, lane_offset=c["lane_offset"],
                  done_list=c["done_list"], episode_stats=c["episode_stats"], final_obs=c["final_obs"], max_episode_steps=c["max_episode_steps"],
                  double_buffer=c["double_buffer"], resident=c["resident"])
        if c["ext"]:                                 # the observation buffer (for CartPole: the state buffer itself), a pair when double buffered
            stride = self.n + PAD
            self.ext = [torch.zeros(self.O * stride + TAIL, dtype=torch.float32, device="cuda") for _ in range(2 if c["double_buffer"] else 1)]
            torch.cuda.synchronize()
            kw.update(ext_obs=self.ext[0], ext_obs_stride=stride)
            if c["double_buffer"]:
                kw["ext_obs_alt"] = self.ext[1]
        env = self.pkg.VectorEnv(c["gym"], c["n"], **kw)
        if c["ext"]:                                 # (create zeroes through the pad columns of all rows but the last: paint afterwards)
            env.Sync()
            for part in self.pads():
                part.fill_(SENTINEL)
            torch.cuda.synchronize()
            self.check_view(env)
        return env

    def check_view(self, env):
        v, ptrs = env.DeviceView(), [b.data_ptr() for b in self.ext]
        assert v.d_obs in ptrs and v.obs_stride == self.n + PAD, "the observation view does not point into the caller's buffer"
        if len(ptrs) == 2:
            assert v.d_obs_alt in ptrs and v.d_obs_alt != v.d_obs
        if H.M.ENVS[self.c["env"]]["alias"]:
            assert v.d_state == v.d_obs

    def pads(self):
        stride = self.n + PAD
        return [p for b in self.ext for p in (b[:self.O * stride].view(self.O, stride)[:, self.n:], b[self.O * stride:])]

    def close(self):
        try:
            if self.ext:
                self.env.Sync()
                self.check_view(self.env)
                for part in self.pads():
                    assert (part.cpu().numpy() == SENTINEL).all(), "a pad column or the tail past the last row of the caller's buffer was written"
        finally:
            self.env.Close()

    def gray(self):
        out = self.torch.empty((self.n, A.SIZE[1], A.SIZE[0]), dtype=self.torch.uint8, device="cuda")
        self.env.RenderDevice(out, "gray", crop=A.CROP, size=A.SIZE)
        self.env.Sync()
        return out.cpu().numpy()

    def mask(self, m):
        self.keep_mask = None if m is None else self.device(m)
        return self.keep_mask

    def host(self, t):
        self.env.Sync()
        self.torch.cuda.synchronize()
        return t.cpu().numpy()

    # -- one attachment operation on the handle ------------------------------------------------------------------------------------
    def attach(self, op):
        env, n, k, torch, m = self.env, self.n, op["kind"], self.torch, self.model
        f32 = lambda *shape: torch.full(shape, 7.25, dtype=torch.float32, device="cuda")      # noqa: E731
        if k == "reconfig":
            v = A.VARIANTS[op["which"]][op["variant"]]
            if op["which"] == "actor":
                self.actor = env.Actor(A.net_of(1, v["S"], v["hidden"], self.A, self.O)[2], history=v["S"])
                if self.c["critic"]:
                    self.actor.SetCritic(A.net_of(2, v["S"], v["hidden"], 1, self.O)[2])
                if self.box:
                    self.actor.SetPolicy(*A.BOX_POLICY)
                else:
                    self.actor.SetExploration(*self.c["explore"])
            elif op["which"] == "stack":
                self.stack = env.PixelStack(depth=v["depth"], size=A.SIZE, crop=A.CROP, format="gray8")
            else:
                self.memory = env.EpisodeMemory(capacity=v["capacity"], max_length=self.c["max_length"], history=v["history"], rollout_chunk=v["chunk"])
            return {}
        if k == "act":
            out = f32(n) if self.box else torch.full((n,), -9, dtype=torch.int32, device="cuda")
            logits, logp = f32(n, self.A), None if self.box else f32(n)
            value = f32(n) if self.c["critic"] else None
            torch.cuda.synchronize()
            self.outs = [t for t in (out, logits, logp, value) if t is not None]
            if self.box:                             # (a Box actor's Act takes no value=: Value() serves it, over the same current history)
                self.actor.Act(op["eps"], op["seed"], op["tick"], out=out, logits=logits)
                if value is not None:
                    self.actor.Value(out=value)
            else:
                self.actor.Act(op["eps"], op["seed"], op["tick"], out=out, logits=logits, logp=logp, value=value)
            return dict(actions=self.host(out), logits=self.host(logits), logp=None if logp is None else self.host(logp),
                        value=None if value is None else self.host(value))
        if k in ("value", "boot"):
            out = f32(n)
            torch.cuda.synchronize()
            self.outs = [out]
            (self.actor.Value if k == "value" else self.actor.Boot)(out=out)
            return dict(out=self.host(out))
        if k == "actor_push":
            self.actor.Push()
        elif k == "actor_reset":
            self.actor.Reset(self.mask(op["mask"]))
        elif k == "actor_load":
            self.actor.Load(A.net_of(op["net_seed"], m.S, A.VARIANTS["actor"][m.variant["actor"]]["hidden"], self.A, self.O)[2])
        elif k == "actor_step":
            return dict(actions=self.host(self.actor.Step(op["eps"], op["seed"], op["tick"])).copy())
        elif k == "actor_rollout":
            T = op["T"]
            rec = dict(rec_obs=torch.zeros((T, self.O, n), dtype=torch.float32, device="cuda"), rec_reward=torch.zeros((T, n), dtype=torch.float32, device="cuda"),
                       rec_done=torch.zeros((T, n), dtype=torch.uint8, device="cuda"),
                       rec_actions=f32(T, n) if self.box else torch.full((T, n), -9, dtype=torch.int32, device="cuda"))
            torch.cuda.synchronize()
            self.outs = [rec["rec_actions"]]
            env.RolloutFusedDevice(None, T, actions="actor", epsilon=op["eps"], action_seed=op["seed"], action_tick0=op["tick"], **rec)
            return dict(fused={k_: self.host(v) for k_, v in rec.items()})
        elif k == "stack_push":
            self.stack.Push()
        elif k == "stack_reset":
            self.stack.Reset(self.mask(op["mask"]))
        elif k == "mem_push":
            a = m.last_a if m.last_a is not None else np.zeros(n, self.adtype)
            self.keep = self.device(np.asarray(a, self.adtype))
            self.memory.Push(self.keep)
        elif k == "mem_reset":
            self.memory.Reset(self.mask(op["mask"]), clear=op["clear"])
        elif k == "mem_rollout":
            ring = np.zeros((op["T"], self.stride), self.adtype)
            ring[:, :n] = op["ring"]
            self.keep = self.device(ring)
            self.memory.Rollout(op["T"], self.keep, action_stride=self.stride, ring=op["T"])
        else:
            raise KeyError(k)
        return {}

    def compare_attachments(self, dataset):
        m = self.model
        if self.actor is not None:
            import ctypes as C
            p, stride, slot = C.c_void_p(), C.c_int64(), C.c_int32()
            assert self.env._lib.gymnet_vecenv_actor_view(self.env._h, C.byref(p), C.byref(stride), C.byref(slot)) == 0
            assert slot.value == m.slot, f"{self.where()}: ring slot {slot.value}, model {m.slot}"
            self.same("actor history", self.actor.History(), m.hist.h)
        if self.stack is not None:
            self.same("pixel stack", self.stack.Read(), m.stack.stack)
        if self.memory is not None:
            mm = m.memory
            s = self.memory.Stats()
            want = dict(kept=len(mm.pool), ended=mm.ended, admitted=mm.admitted, too_long=mm.too_long)
            assert s == want, f"{self.where()}: memory stats {s}, model {want}"
            for g, w, what in zip(self.memory.Episodes(), mm.kept(), ("return", "length", "end_tick", "lane")):
                self.same(f"kept episodes' {what}", g, w)
            if dataset:
                x, a, onehot, r = mm.dataset_params(None if self.box else self.A)
                assert self.memory.DatasetSize() == len(x), f"{self.where()}: dataset rows {self.memory.DatasetSize()}, model {len(x)}"
                if len(x):
                    gx, ga, go, gr = (None if v is None else v.cpu().numpy() for v in self.memory.BuildDataset("params", min_episodes=0, reward=True))
                    self.same("dataset x", gx, x)
                    self.same("dataset actions", ga, a.astype(self.adtype))
                    assert (go is None) == (onehot is None)
                    if go is not None:
                        self.same("dataset one-hot", go, onehot)
                    self.same("dataset rewards", gr, r)

    def compare_outputs(self, k, got, rec):
        if k == "act":
            self.same("act actions", got["actions"], rec["actions"])
            assert twin.same(got["logits"], rec["logits"]), f"{self.where()}: logits differ from the twin"
            if rec["logp"] is not None:
                self.same("act logp", got["logp"].view(np.uint32), rec["logp"])
            if rec["value"] is not None:
                assert twin.same(got["value"], rec["value"]), f"{self.where()}: values differ from the twin"
        elif k in ("value", "boot"):
            assert twin.same(got["out"], rec), f"{self.where()}: {k} differs from the twin"
        elif k == "actor_step":
            self.same("actor_step actions", got["actions"], rec[0]["act"]["actions"])
        elif k == "actor_rollout":
            f = got["fused"]
            for t, want in enumerate(rec):
                self.same(f"recorded action, step {t}", f["rec_actions"][t], want["act"]["actions"])
                self.same(f"recorded observation, step {t}", f["rec_obs"][t], want["obs"])
                self.same(f"recorded reward, step {t}", f["rec_reward"][t], want["reward"])
                self.same(f"recorded done, step {t}", f["rec_done"][t], want["done"])

    # -- one operation, both sides ---------------------------------------------------------------------------------------------------
    def run(self, i, op, last=False):
        self.i, self.op = i, op
        k = op["kind"]
        served = False
        if k in A.HANDLE_KINDS:
            if k == "set_tick" and op["value"] == "same":
                op = dict(op, value=self.env.Tick)
            try:
                got = self.call(op)
            except base.REFUSED as e:
                pytest.fail(f"{self.where()}: the library refused a call the table accepts: {e!r}")
            _, recs = A.apply(self.model, op, self.mslots)
            self.returned(got.get("obs"), got.get("reward"), got.get("done"), got.get("truncated"))
            served = (k == "step" and op["path"] in ("Step", "StepInt", "StepInto")) or (k == "reset" and op["path"] == "Reset")
            if "fused" in got:
                self.compare_fused(got, recs)
        elif k in ("stack_push", "stack_reset") or (k == "reconfig" and op["which"] == "stack"):
            self.attach(op)                          # (never refused; the model takes the frame the handle shows afterwards)
            A.apply(self.model, op, self.mslots, gray=self.gray())
        else:
            self.outs = []
            ok, rec = A.apply(self.model, op, self.mslots)
            if ok:
                try:
                    got = self.attach(op)
                except ValueError as e:
                    pytest.fail(f"{self.where()}: the library refused a call the staleness rules accept: {e}")
                self.compare_outputs(k, got, rec)
            else:
                with pytest.raises(ValueError, match=r"^" + A.PREFIX[k]) as e:
                    self.attach(op)
                    pytest.fail(f"{self.where()}: the library accepted a call the staleness rules refuse")
                assert "gymnet status -1" in str(e.value), f"{self.where()}: {e.value}"
                for t in self.outs:                  # nothing written
                    got = self.host(t)
                    assert (got == (7.25 if got.dtype == np.float32 else -9)).all(), f"{self.where()}: a refused call wrote its output"
        full = not self.c["resident"] or not served or i % 3 == 2
        self.compare(full)
        if full:
            self.compare_attachments(dataset=last or i % 8 == 7)
        if full and self.c["done_list"] and self.model.last_fin is not None and (k in H.STEP_LIKE or k in ("actor_step", "actor_rollout", "mem_rollout")):
            self.compare_done_list()


def _run(gpu_pkg, oracle, name, ops):
    d = Driver(gpu_pkg, oracle, name)
    try:
        for i, op in enumerate(ops):
            d.run(i, op, last=i == len(ops) - 1)
    finally:
        d.close()


@pytest.mark.parametrize("seed", AQ.MIXED_SEEDS)
@pytest.mark.parametrize("name", sorted(A.CONFIGS))
def test_a_mixed_sequence_leaves_handle_and_attachments_equal_to_the_model(gpu_pkg, oracle, name, seed):
    _run(gpu_pkg, oracle, name, AQ.mixed(name, seed))


@pytest.mark.parametrize("name", sorted(A.CONFIGS))
def test_every_staleness_refusal_is_held_to_the_library(gpu_pkg, oracle, name):
    """Scripted: after each event that leaves the attachments stale every gate refuses, the resets cure, the accepted calls are compared."""
    _run(gpu_pkg, oracle, name, AQ.table(name))
