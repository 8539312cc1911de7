"""What the attachment sequences cover, asserted from the data and the CPU model alone (no GPU): tests/_attachment_sequences.py run through
tests/_attachment_replay.py AttachedModel with an all-background frame in place of the handle's render.

  every operation kind a configuration takes occurs ACCEPTED in its sequences, and every refusal of the staleness rules occurs REFUSED
  in its table; in every mixed sequence at least one accepted push restarts some lanes while others append, and both done bits occur
  where the configuration has a time limit (Pendulum, which has no terminal state: the time-limit bit); in every configuration's mixed
  sequences a Seed and a Restore each fall between an attachment event and a gated call that is then refused, with no step-like call in
  between; the keyed configuration's prologue leaves per-lane keys installed.  These are conditions, not measurements: the seeds are chosen so that they hold."""
import numpy as np
import pytest

import _attachment_replay as A
import _attachment_sequences as AQ

GATED = {"act": "actor", "value": "actor", "boot": "actor", "actor_push": "actor", "actor_step": "actor", "actor_rollout": "actor",
         "mem_push": "memory", "mem_rollout": "memory"}


def _replay(oracle, name, ops):
    """[(op, accepted, done bytes after it or None, handle kinds since the gate's last event)]"""
    c = A.CONFIGS[name]
    m = A.AttachedModel(oracle, c)
    gray = np.full((c["n"], A.SIZE[1], A.SIZE[0]), 255, np.uint8)
    slots, out = {}, []
    since = {"actor": [], "memory": []}
    gate_ids = {k: id(g) for k, g in m.gate.items()}
    for op in ops:
        k = op["kind"]
        before = {w: list(v) for w, v in since.items()}
        ok, _ = A.apply(m, op, slots, gray=gray)
        if k in A.HANDLE_KINDS or k in ("actor_step", "actor_rollout", "mem_rollout"):      # (the latter step the handle where they run)
            for v in since.values():
                v.append(k)
        for w, g in m.gate.items():
            if id(g) != gate_ids[w]:
                gate_ids[w], since[w] = id(g), []
        stepped = k in ("step", "decision", "rollout", "actor_step", "actor_rollout", "mem_rollout")
        out.append((op, ok, m.done.copy() if stepped or k in ("actor_push", "mem_push") else None, before.get(GATED.get(k), [])))
    return out


@pytest.fixture(scope="module")
def runs(oracle):
    return {name: dict(table=_replay(oracle, name, AQ.table(name)), mixed=[_replay(oracle, name, AQ.mixed(name, s)) for s in AQ.MIXED_SEEDS])
            for name in A.CONFIGS}


def test_the_sequences_are_pure_data_of_the_stated_length():
    for name in A.CONFIGS:
        for s in AQ.MIXED_SEEDS:
            a, b = AQ.mixed(name, s), AQ.mixed(name, s)
            assert len(a) == AQ.MIXED_OPS and [op["kind"] for op in a] == [op["kind"] for op in b]
            assert {op["kind"] for op in a} <= set(A.HANDLE_KINDS) | A.kinds_of(A.CONFIGS[name])


@pytest.mark.parametrize("name", sorted(A.CONFIGS))
def test_every_accepted_kind_occurs_in_every_configuration(runs, name):
    c = A.CONFIGS[name]
    seen = {op["kind"] for r in [runs[name]["table"]] + runs[name]["mixed"] for op, ok, _, _ in r if ok}
    handle = set(A.HANDLE_KINDS) - (set() if c["max_episode_steps"] else {"set_array"})       # (the lengths are set where a limit exists)
    assert (handle | A.kinds_of(c)) - seen == set()


@pytest.mark.parametrize("name", sorted(A.CONFIGS))
def test_every_refusal_occurs_in_the_table(runs, name):
    c = A.CONFIGS[name]
    refused = {op["kind"] for op, ok, _, _ in runs[name]["table"] if not ok}
    want = {k for k in A.PREFIX if k in A.kinds_of(c)}
    assert want - refused == set()
    assert refused <= set(A.PREFIX)
    # and every event that leaves the attachments stale is followed by a refused act
    kinds = [(op["kind"], ok) for op, ok, _, _ in runs[name]["table"]]
    assert sum(1 for (k, ok) in kinds if k == "act" and not ok) >= len(AQ.STALE_EVENTS)
    if c["resident"]:                               # a served host step: the push is refused, a StepDevice step's is accepted
        pushes = [ok for (op, ok, _, _) in runs[name]["table"] if op["kind"] == "actor_push"]
        assert pushes[-2:] == [False, True]


@pytest.mark.parametrize("seed", range(len(AQ.MIXED_SEEDS)))
@pytest.mark.parametrize("name", sorted(A.CONFIGS))
def test_a_mixed_sequence_pushes_restarting_and_appending_lanes_together(runs, name, seed):
    c = A.CONFIGS[name]
    r = runs[name]["mixed"][seed]
    mixed = [d for op, ok, d, _ in r if ok and op["kind"] in ("actor_push", "mem_push", "actor_step", "actor_rollout") and (d != 0).any() and (d == 0).any()]
    assert mixed, "no accepted push restarts some lanes while others append"
    if c["max_episode_steps"]:
        bits = np.bitwise_or.reduce(np.concatenate([d for _, _, d, _ in r if d is not None]))
        assert bits & 2
        assert bits & 1 or c["env"] == "Pendulum"    # (Pendulum has no terminal state: its episodes end by the time limit alone)
    assert any(not ok for _, ok, _, _ in r) and sum(ok for op, ok, _, _ in r if op["kind"] in GATED) >= 5


@pytest.mark.parametrize("name", sorted(A.CONFIGS))
def test_a_seed_and_a_restore_fall_between_an_attachment_event_and_a_refused_call(runs, name):
    """... and are its cause: no step-like call lies between the attachment event and the refused call, so the gate was not stale anyway"""
    stepping = {"step", "decision", "rollout", "actor_step", "actor_rollout", "mem_rollout"}
    causes = set()
    for r in runs[name]["mixed"]:
        for op, ok, _, since in r:
            if op["kind"] in GATED and not ok and not stepping & set(since):
                causes |= set(since)
    assert {"seed", "restore"} <= causes, causes


def test_the_keyed_configuration_runs_on_per_lane_keys(oracle):
    keyed = [name for name, c in A.CONFIGS.items() if c["keys"]]
    assert keyed
    for name in keyed:
        m, slots = A.AttachedModel(oracle, A.CONFIGS[name]), {}
        for op in AQ.prologue(A.CONFIGS[name], np.random.default_rng(0)):
            A.apply(m, op, slots, gray=None)
        assert m.seeds is not None and len(np.unique(m.seeds)) >= 2 and m.hist is not None
