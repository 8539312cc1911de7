"""Call sequences over a handle WITH its attachments (pure data, seeded, no GPU; helper module, not a conftest).  The handle kinds are
those of tests/_call_sequences.py and use its ingredients; beside them:

  act, value, boot                     compared with the twins over the model's history; refused where the staleness state says so
  actor_push, actor_reset(mask|None), actor_step, actor_load, actor_rollout (fused, T in 1..6)
  stack_push, stack_reset(mask|None)
  mem_push, mem_reset(mask|None, clear), mem_rollout
  reconfig                             one attachment replaced while the others live

table(name): scripted — every documented refusal of the staleness rules, each followed by the reset that cures it and a compared accepted
call.  mixed(name, seed): 48 operations; a light copy of the staleness state (tests/_attachment_replay.py Gate, advance) steers the draw so
that pushes mostly follow single steps and resets mostly follow the calls that leave an attachment stale — and sometimes do not."""
import numpy as np

import _attachment_replay as A
import _call_sequences as Q

MIXED_SEEDS = (0, 1, 2)
MIXED_OPS = 48
CONFIGS = A.CONFIGS


def _act(rng, kind="act", **more):
    return dict(kind=kind, eps=float(rng.choice([0.0, 0.25, 1.0])), seed=int(rng.integers(1, 2 ** 40)), tick=int(rng.integers(0, 2 ** 33)), **more)


def _mask(c, rng):
    return None if rng.random() < 0.4 else Q.lane_mask(c, rng)


def _step(c, rng, path="StepDevice"):
    return Q.op_step(c, rng, path=path)


def _lengths(c, rng):
    """running episode lengths drawn per lane, so that the time limit strikes a few lanes in every step (a reset zeroes them all)"""
    return [dict(kind="set_array", name="episode_length", value=Q.lengths(c, rng))] if c["max_episode_steps"] else []


def prologue(c, rng):
    ops = [Q.op_reset(c, rng, "Reset")] + ([Q.op_seed(c, rng, "keys"), Q.op_reset(c, rng, "Reset")] if c["keys"] else [])
    ops += [dict(kind="set_state", state=Q.edge_state(c, rng))] + _lengths(c, rng)
    ops += [dict(kind="reconfig", which=w, variant=0) for w in ("actor", "stack", "memory") if w == "actor" or c[w]]
    return ops


def _resets(c, rng, masked=True):
    """the resets that cure every attachment (the stack has no gate, it is reset for its content)"""
    m = (lambda: _mask(c, rng)) if masked else (lambda: None)
    ops = [dict(kind="actor_reset", mask=m())]
    if c["stack"]:
        ops.append(dict(kind="stack_reset", mask=m()))
    if c["memory"]:
        ops.append(dict(kind="mem_reset", mask=m(), clear=bool(rng.random() < 0.2)))
    return ops


def _pushes(c, rng):
    """what follows one single step, in a drawn order (a boot goes before the actor's push)"""
    ops = [["actor_push"]]
    if "boot" in A.kinds_of(c):
        ops[0].insert(0, "boot")
    if c["stack"]:
        ops.append(["stack_push"])
    if c["memory"]:
        ops.append(["mem_push"])
    return [dict(kind=k) for i in rng.permutation(len(ops)) for k in ops[i]]


def _other_pushes(c):
    """after actor_step, which pushes the actor itself"""
    return [dict(kind=k) for k, on in (("stack_push", c["stack"]), ("mem_push", c["memory"])) if on]


# ---- the table ---------------------------------------------------------------------------------------------------------------
STALE_EVENTS = ("step_step", "reset", "reset_where", "seed", "seed_keys", "set_lane_seeds", "set_tick_same", "set_tick_jump", "set_state", "restore",
                "seed_reset_to_the_marked_tick", "rollout_fused", "decision4")


def _event(c, rng, what):
    if what == "step_step":
        return [_step(c, rng), _step(c, rng, "Step")]
    if what == "reset":
        return [Q.op_reset(c, rng, "ResetDevice")]
    if what == "reset_where":
        return [dict(kind="reset_where", path="ResetWhereDevice", mask=Q.lane_mask(c, rng))]
    if what == "seed":
        return [Q.op_seed(c, rng, "int")]
    if what == "seed_keys":
        return [Q.op_seed(c, rng, "keys")]
    if what == "set_lane_seeds":
        return [dict(kind="set_lane_seeds", value=Q.lane_keys(c, rng))]
    if what == "set_tick_same":
        return [dict(kind="set_tick", value="same")]
    if what == "set_tick_jump":
        return [dict(kind="set_tick", value=Q.TICK_JUMP)]
    if what == "set_state":
        return [dict(kind="set_state", state=Q.edge_state(c, rng))]
    if what == "restore":
        return [dict(kind="checkpoint", slot="t"), dict(kind="restore", slot="t")]
    if what == "seed_reset_to_the_marked_tick":    # Seed; Reset; attachments marked at tick 1; Seed; Reset: tick 1 again
        return [Q.op_seed(c, rng, "int"), Q.op_reset(c, rng, "Reset")] + _resets(c, rng, masked=False) + [Q.op_seed(c, rng, "int"), Q.op_reset(c, rng, "Reset")]
    if what == "rollout_fused":
        return [Q.op_rollout(c, rng, "fused", 3, 3)]
    if what == "decision4":
        return [Q.op_decision(c, rng, "StepRepeatDevice", 4), Q.op_decision(c, rng, "StepRepeatDevice", 2)]
    raise KeyError(what)


def table(name):
    c = CONFIGS[name]
    rng = np.random.default_rng([98, sum(map(ord, name))])
    kinds = A.kinds_of(c)
    ops = prologue(c, rng)
    for what in STALE_EVENTS:
        ops += _event(c, rng, what)
        # every gate refuses ...
        ops += [_act(rng), dict(kind="actor_push"), _act(rng, "actor_step")] + ([_act(rng, "actor_rollout", T=2)] if "actor_rollout" in kinds else [])
        ops += [dict(kind=k) for k in ("value", "boot", "mem_push") if k in kinds]
        # ... the resets cure, and the accepted calls are compared
        ops += _resets(c, rng, masked=False)
        ops += [_act(rng)] + ([dict(kind="value")] if "value" in kinds else [])
        ops += [_step(c, rng)] + _pushes(c, rng)
    # the refusals that are no staleness: a push without a step, an act after a step
    ops += [dict(kind="actor_push")] + ([dict(kind="mem_push")] if c["memory"] else []) + [_step(c, rng), _act(rng)] + _pushes(c, rng)
    if c["memory"]:                                 # a rollout ingest on a memory that missed a push: the launch runs, the ingest is refused
        ops += [_step(c, rng), dict(kind="mem_rollout", T=3, ring=Q.ring_of(c, rng, 3))] + _resets(c, rng, masked=False)
        ops += [dict(kind="mem_rollout", T=5, ring=Q.ring_of(c, rng, 5))]
    if c["resident"]:                               # a host step the resident kernel serves: a tick, no step launch
        ops += _resets(c, rng, masked=False) + [_step(c, rng, "Step"), dict(kind="actor_push")] + _resets(c, rng, masked=False)
        ops += [_step(c, rng, "StepDevice"), dict(kind="actor_push")]
    for w in ("actor", "stack", "memory"):
        if w == "actor" or c[w]:
            ops += [dict(kind="reconfig", which=w, variant=1), _act(rng, "actor_step")] + _other_pushes(c)
    ops += [dict(kind="actor_load", net_seed=7), _act(rng)] + ([_act(rng, "actor_rollout", T=6), _act(rng)] if "actor_rollout" in kinds else [])
    return ops


# ---- mixed -------------------------------------------------------------------------------------------------------------------
def mixed(name, seed):
    c = CONFIGS[name]
    rng = np.random.default_rng([seed, sum(map(ord, name)), 7])
    kinds = A.kinds_of(c)
    ops = prologue(c, rng)
    gates = [A.Gate(), A.Gate()]                    # the actor's and the memory's, as the model will see them
    variant = {"actor": 0, "stack": 0, "memory": 0}
    have_ck = False
    # one of each, in a drawn order, and draws for the rest
    must = ["set_tick", "set_state", "set_lane_seeds", "reset", "reset_where", "decision", "rollout", "actor_load", "reconfig", "actor_step", "act"]
    must += [k for k in ("actor_rollout", "mem_rollout", "value") if k in kinds]
    must = [must[i] for i in rng.permutation(len(must))] + ["restore", "seed", "kick"]       # (popped from the end: these three come first)

    first = list(must)

    def emit(op):
        ops.append(op)
        k = op["kind"]
        if k in A.HANDLE_KINDS:
            A.advance(gates, op, c)
        elif k in ("actor_reset", "actor_push"):
            gates[0] = A.Gate() if (k == "actor_reset" or gates[0].one_launch_of(1)) else gates[0]
        elif k in ("mem_reset", "mem_push"):
            gates[1] = A.Gate() if (k == "mem_reset" or gates[1].one_launch_of(1)) else gates[1]
        elif k in ("actor_step", "actor_rollout"):
            if gates[0].current():
                T = 1 if k == "actor_step" else op["T"]
                gates[1].stepped(T, 1)
                gates[0] = A.Gate()
        elif k == "mem_rollout":
            ok = gates[1].current()
            for g in gates:
                g.stepped(op["T"], 1)
            if ok:
                gates[1] = A.Gate()
        elif k == "reconfig" and op["which"] != "stack":
            gates[0 if op["which"] == "actor" else 1] = A.Gate()

    def draw(k):
        nonlocal have_ck
        if k == "kick":                             # lanes put next to termination, the attachments reset, one step, every push
            return [dict(kind="set_state", state=Q.edge_state(c, rng))] + _resets(c, rng, masked=False) + [_step(c, rng)] + _pushes(c, rng)
        if k == "seed":                             # the ordinary re-seeding idiom, and the call that must then be refused
            return [Q.op_seed(c, rng), Q.op_reset(c, rng)] + _lengths(c, rng) + [_act(rng)]
        if k == "restore":
            pre = [] if have_ck else [dict(kind="checkpoint", slot="m"), _step(c, rng)] + _pushes(c, rng)
            have_ck = True
            return pre + [dict(kind="restore", slot="m"), dict(kind="actor_push") if rng.random() < 0.5 else _act(rng)]
        if k == "set_tick":
            return [dict(kind="set_tick", value=Q.TICK_JUMP if rng.random() < 0.5 else "same")]
        if k == "set_state":
            return [dict(kind="set_state", state=Q.edge_state(c, rng))]
        if k == "set_lane_seeds":
            return [dict(kind="set_lane_seeds", value=Q.lane_keys(c, rng))]
        if k == "reset":
            return [Q.op_reset(c, rng)] + _lengths(c, rng)
        if k == "reset_where":
            return [Q.op_reset_where(c, rng)]
        if k == "decision":
            return [Q.op_decision(c, rng, R=int(rng.choice([2, 4])))] + _pushes(c, rng)
        if k == "rollout":
            return [Q.op_random_rollout(c, rng)]
        if k == "actor_rollout":
            return [_act(rng, "actor_rollout", T=int(rng.integers(1, 7)))]
        if k == "actor_load":
            return [dict(kind="actor_load", net_seed=int(rng.integers(3, 99)))]
        if k == "reconfig":
            which = [w for w in ("actor", "stack", "memory") if w == "actor" or c[w]]
            w = which[rng.integers(0, len(which))]
            variant[w] ^= 1
            return [dict(kind="reconfig", which=w, variant=variant[w])]
        if k == "actor_step":
            return [_act(rng, "actor_step")] + _other_pushes(c)
        if k == "act":
            return [_act(rng)]
        if k == "value":
            return [dict(kind="value")]
        if k == "mem_rollout":
            T = int(rng.integers(2, 7))
            return [dict(kind="mem_rollout", T=T, ring=Q.ring_of(c, rng, T))]
        if k == "step":
            return [_step(c, rng, path=None)] + (_pushes(c, rng) if rng.random() < 0.85 else [])
        raise KeyError(k)

    while len(ops) < MIXED_OPS:
        stale = not gates[0].current() or (c["memory"] and not gates[1].current())
        if stale and rng.random() < 0.85:
            batch = _resets(c, rng)
        elif must and (len(must) > len(first) - 3 or rng.random() < 0.4):
            batch = draw(must.pop())
        else:
            batch = draw(("step", "step", "step", "actor_step", "act")[rng.integers(0, 5)])
        for op in batch:
            emit(op)
    return ops[:MIXED_OPS]
