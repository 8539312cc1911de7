"""The staleness table of the actor and the episode memory: every gate of include/gymnet_amd.h's staleness rules crossed with every
event that may fall between an attachment event (config / reset / push / actor rollout) and the gated call.

The expected outcome of each cell is written by hand from the header, NOT derived from the library:

  act / value / a fused actor rollout   accepted iff the history is current: no vector step since the attachment event, and none of
                                        the calls the header lists as leaving the history stale (a reset of the handle that launches,
                                        seed, seed_lanes, set_tick, set_state, restoring a checkpoint).
  actor push / boot                     accepted iff exactly one vector step (one decision in one step launch) ran since then and none of
                                        the listed calls.
  memory push                           the same rule, on the memory's own last config / reset / push.
  memory push_rollout(steps)            accepted iff exactly one step launch of `steps` decisions ran since then and none of the listed calls.

A RolloutDevice of one step IS one vector step in one launch, so the pushes take it; a frame-skip decision (StepRepeatDevice) is one
decision.  ResetWhere(None) on an auto-reset handle is the documented no-op: nothing goes stale.  `Tick = the same value` is set_tick,
and set_tick is on the list whatever value it stores.

A refused call returns GYMNET_ERR_INVALID_ARG (ValueError here) with the unit's message and changes nothing: the history and its ring
slot, the memory's stats and kept episodes, the handle's state, tick and done bytes, and the poisoned output buffer are compared before
and after.  An accepted call must not raise.

The compound events are the ones that returned the handle's (tick, step launches) pair to where an attachment had marked it:
Seed; Reset — Reset; Tick = mark — a rollout; Tick = mark + 1 — each also with a following single step for the push gates."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 0x57A1E
N = 259                      # four waves and three lanes
S = 2
LIMIT = 9
POISON = -7.0

OK, NO = True, False
# event -> (act-like gates, actor push / boot, memory push, memory push_rollout, the steps push_rollout asks for)
TABLE = {
    "nothing":                  (OK, NO, NO, NO, 1),
    "step":                     (NO, OK, OK, OK, 1),
    "two_steps":                (NO, NO, NO, NO, 2),
    "rollout_1":                (NO, OK, OK, OK, 1),
    "fused_ring_3":             (NO, NO, NO, OK, 3),
    "fused_actor_3":            (OK, NO, NO, OK, 3),
    "repeat_3":                 (NO, OK, OK, OK, 1),
    "reset":                    (NO, NO, NO, NO, 1),
    "reset_device":             (NO, NO, NO, NO, 1),
    "reset_where_device_mask":  (NO, NO, NO, NO, 1),
    "reset_where_none_noop":    (OK, NO, NO, NO, 1),
    "step_reset_where_none_noop": (NO, OK, OK, OK, 1),
    "seed":                     (NO, NO, NO, NO, 1),
    "seed_lanes":               (NO, NO, NO, NO, 1),
    "tick_same":                (NO, NO, NO, NO, 1),
    "tick_other":               (NO, NO, NO, NO, 1),
    "set_state":                (NO, NO, NO, NO, 1),
    "restore_now":              (NO, NO, NO, NO, 1),
    "restore_older":            (NO, NO, NO, NO, 1),
    # the compound events
    "seed_reset":               (NO, NO, NO, NO, 1),
    "reset_tick_mark":          (NO, NO, NO, NO, 1),
    "fused_ring_3_tick_mark_plus_1": (NO, NO, NO, NO, 1),
    "fused_ring_3_tick_mark_plus_3": (NO, NO, NO, NO, 3),
    "seed_reset_step":          (NO, NO, NO, NO, 1),
    "reset_tick_mark_step":     (NO, NO, NO, NO, 1),
    "set_state_step":           (NO, NO, NO, NO, 1),
    "tick_same_step":           (NO, NO, NO, NO, 1),
    "step_tick_same":           (NO, NO, NO, NO, 1),
    "step_set_state":           (NO, NO, NO, NO, 1),
    "seed_lanes_reset_step":    (NO, NO, NO, NO, 1),
    "restore_now_step":         (NO, NO, NO, NO, 1),
    # the most ordinary idiom: Seed; Reset; attachments marked at tick 1 — then Seed; Reset again brings tick 1 back
    "marked_at_1_seed_reset":       (NO, NO, NO, NO, 1),
    "marked_at_1_seed_reset_step":  (NO, NO, NO, NO, 1),
}
GATES = {"act": 0, "act_value": 0, "value": 0, "fused_actor": 0, "actor_push": 1, "boot": 1, "mem_push": 2, "mem_push_rollout": 3}
# what a refusal of the gate says (the unit's wording)
MESSAGE = {"act": "the actor's history is stale", "act_value": "the actor's history is stale", "value": "the actor's history is stale",
           "fused_actor": "the actor's history is stale", "actor_push": "an actor push needs exactly one vector step",
           "boot": "an actor boot needs exactly one vector step", "mem_push": "a push needs exactly one vector step since the last memory",
           "mem_push_rollout": "a push needs exactly one vector step since the last memory"}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _net(rng, widths):
    return [(rng.normal(0, 1, (o, i)).astype(np.float32), rng.normal(0, 1, o).astype(np.float32)) for i, o in zip(widths[:-1], widths[1:])]


class Rig:
    """One auto-reset CartPole handle with a time limit and dense terminal observations (what Boot reads), an actor with a critic and
    an episode memory with a rollout chunk; prepare() brings all of them to a fresh, marked position."""

    def __init__(self, pkg):
        import torch
        self.torch = torch
        rng = np.random.default_rng(5)
        self.env = pkg.VectorEnv("CartPole-v1", N, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=LIMIT, final_obs=True)
        self.env.Reset()
        self.actor = self.env.Actor(_net(rng, [S * 4, 8, 2]), history=S)
        self.actor.SetCritic(_net(rng, [S * 4, 8, 1]))
        self.mem = self.env.EpisodeMemory(capacity=4, max_length=0, history=S, rollout_chunk=4)
        self.rng = rng
        self.ring = _dev(rng.integers(0, 2, (3, N)).astype(np.int32))
        self.rec = (torch.zeros((3, 4, N), dtype=torch.float32, device="cuda"), torch.zeros((3, N), dtype=torch.float32, device="cuda"),
                    torch.zeros((3, N), dtype=torch.uint8, device="cuda"), torch.zeros((3, N), dtype=torch.int32, device="cuda"))
        self.older = None

    def close(self):
        self.env.Close()

    def step(self):
        self.env.StepDevice(self.ring[0])

    def prepare(self):
        """a few steps (so that the launch count and the tick are not small round numbers and an older checkpoint exists), then a reset
        of the handle and of both attachments: the marked position"""
        env = self.env
        env.Seed(SEED)
        env.Reset()
        self.step()
        self.older = env.Checkpoint()
        self.step()
        env.Reset()
        self.actor.Reset()
        self.mem.Reset(clear=True)
        self.mark = env.Tick

    # ---- the events ------------------------------------------------------------------------------------------------------------
    def event(self, name):
        env, ring, (obs, rew, done, act) = self.env, self.ring, self.rec
        mask = _dev((np.arange(N) % 3 == 0).astype(np.uint8))
        fused_ring = lambda: env.RolloutFusedDevice(ring, 3, N, 3, rec_obs=obs, rec_reward=rew, rec_done=done)

        def set_state():
            s = env.GetState()
            env.SetState(np.ascontiguousarray(s[:, ::-1]))

        def tick_same():
            env.Tick = env.Tick

        def seed_lanes():
            env.Seed(np.arange(N) % 3 + 11)

        def tick_mark():
            env.Tick = self.mark

        def mark_at_1():                             # (part of the set-up, not of the event: the attachments' marks move to tick 1)
            env.Seed(SEED)
            env.Reset()
            self.actor.Reset()
            self.mem.Reset(clear=True)
            assert env.Tick == 1

        steps = {
            "nothing": [],
            "step": [self.step],
            "two_steps": [self.step, self.step],
            "rollout_1": [lambda: env.RolloutDevice(ring, 1, N, 3)],
            "fused_ring_3": [fused_ring],
            "fused_actor_3": [lambda: env.RolloutFusedDevice(None, 3, actions="actor", epsilon=0.25, action_seed=3, action_tick0=50, rec_obs=obs,
                                                             rec_reward=rew, rec_done=done, rec_actions=act)],
            "repeat_3": [lambda: env.StepRepeatDevice(ring[0], 2)],
            "reset": [env.Reset],
            "reset_device": [env.ResetDevice],
            "reset_where_device_mask": [lambda: env.ResetWhereDevice(mask)],
            "reset_where_none_noop": [lambda: env.ResetWhere(None)],
            "step_reset_where_none_noop": [self.step, lambda: env.ResetWhereDevice(None)],
            "seed": [lambda: env.Seed(5)],
            "seed_lanes": [seed_lanes],
            "tick_same": [tick_same],
            "tick_other": [lambda: setattr(env, "Tick", env.Tick + 7)],
            "set_state": [set_state],
            "restore_now": [lambda: env.Restore(env.Checkpoint())],
            "restore_older": [lambda: env.Restore(self.older)],
            "seed_reset": [lambda: env.Seed(5), env.Reset],
            "reset_tick_mark": [env.Reset, tick_mark],
            "fused_ring_3_tick_mark_plus_1": [fused_ring, lambda: setattr(env, "Tick", self.mark + 1)],
            "fused_ring_3_tick_mark_plus_3": [fused_ring, lambda: setattr(env, "Tick", self.mark + 3)],
            "seed_reset_step": [lambda: env.Seed(5), env.Reset, self.step],
            "reset_tick_mark_step": [env.Reset, tick_mark, self.step],
            "set_state_step": [set_state, self.step],
            "tick_same_step": [tick_same, self.step],
            "step_tick_same": [self.step, tick_same],
            "step_set_state": [self.step, set_state],
            "seed_lanes_reset_step": [seed_lanes, env.Reset, self.step],
            "restore_now_step": [lambda: env.Restore(env.Checkpoint()), self.step],
            "marked_at_1_seed_reset": [mark_at_1, lambda: env.Seed(5), env.Reset],
            "marked_at_1_seed_reset_step": [mark_at_1, lambda: env.Seed(5), env.Reset, self.step],
        }[name]
        for f in steps:
            f()

    # ---- the gates -------------------------------------------------------------------------------------------------------------
    def gate(self, name, steps):
        """returns (call, the poisoned output tensors the call would write)"""
        torch, env, actor, mem = self.torch, self.env, self.actor, self.mem
        f32 = lambda *shape: torch.full(shape, POISON, dtype=torch.float32, device="cuda")
        i32 = lambda *shape: torch.full(shape, -9, dtype=torch.int32, device="cuda")
        if name == "act":
            out, logits = i32(N), f32(N, 2)
            return (lambda: actor.Act(0.25, 3, 4, out=out, logits=logits)), [out, logits]
        if name == "act_value":
            out, logp, v = i32(N), f32(N), f32(N)
            return (lambda: actor.Act(0.25, 3, 4, out=out, logp=logp, value=v)), [out, logp, v]
        if name == "value":
            v = f32(N)
            return (lambda: actor.Value(out=v)), [v]
        if name == "fused_actor":
            acts, v = i32(2, N), f32(2, N)
            return (lambda: env.RolloutFusedDevice(None, 2, actions="actor", epsilon=0.25, action_seed=3, action_tick0=60, rec_actions=acts,
                                                   rec_value=v)), [acts, v]
        if name == "actor_push":
            return actor.Push, []
        if name == "boot":
            b = f32(N)
            return (lambda: actor.Boot(out=b)), [b]
        if name == "mem_push":
            return (lambda: mem.Push(self.ring[0])), []
        if name == "mem_push_rollout":
            obs, rew, done, _ = self.rec
            return (lambda: mem.PushRollout(steps, obs, self.ring, rew, done)), []
        raise KeyError(name)

    def snapshot(self):
        env, actor, mem = self.env, self.actor, self.mem
        import ctypes as C
        p, stride, slot = C.c_void_p(), C.c_int64(), C.c_int32()
        assert env._lib.gymnet_vecenv_actor_view(env._h, C.byref(p), C.byref(stride), C.byref(slot)) == 0
        return dict(history=actor.History(), slot=slot.value, stats=mem.Stats(), episodes=mem.Episodes(), rows=mem.DatasetSize(),
                    state=env.GetState(), tick=env.Tick, done=env.GetArray("done"), reward=env.GetArray("reward"), seed=env.GetSeed(),
                    counters=env.Counters())


def _equal(a, b):
    if isinstance(a, dict) and not isinstance(a, np.ndarray):
        return a.keys() == b.keys() and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    return a == b


@pytest.fixture(scope="module")
def rig(gpu_pkg):
    r = Rig(gpu_pkg)
    yield r
    r.close()


def test_the_table_names_every_gate_family_and_both_outcomes():
    for col in range(4):
        assert {row[col] for row in TABLE.values()} == {OK, NO}
    assert set(GATES.values()) == {0, 1, 2, 3} and set(MESSAGE) == set(GATES)


@pytest.mark.parametrize("gate", list(GATES))
@pytest.mark.parametrize("event", list(TABLE))
def test_cell(rig, event, gate):
    row = TABLE[event]
    want = row[GATES[gate]]
    rig.prepare()
    rig.event(event)
    call, outs = rig.gate(gate, row[4])
    rig.torch.cuda.synchronize()                      # the poison (torch's stream) lands before the handle's stream may write
    if want:
        call()                                        # accepted: must not raise
        rig.env.Sync()
        return
    before = rig.snapshot()
    with pytest.raises(ValueError) as e:
        call()
    assert "gymnet status -1" in str(e.value) and MESSAGE[gate] in str(e.value), str(e.value)
    assert _equal(rig.snapshot(), before), "a refused call changed something"
    for t in outs:                                    # nothing written
        got = _host(t)
        assert (got == (POISON if got.dtype == np.float32 else -9)).all()
