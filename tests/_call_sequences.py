"""Call sequences over one handle (helper module, not a conftest): pure data, seeded, no GPU and no library.

An operation is a dict: "kind" (tests/_handle_replay.py KINDS — what it means to the model), where a kind has several entry points
"path" (which of them the GPU test takes), and its arguments as NumPy arrays.  tests/_handle_replay.py apply() runs one on the model,
tests/test_gpu_call_sequences.py runs it on a handle; tests/test_call_sequences_host.py asserts what the sequences cover.

Three families.
  table(name): scripted, nothing drawn — every refusal of the configuration's table, every launch-policy form it accepts, the no-op
      calls, the three forms of Seed, ResetWhere(None) through both entry points, each followed by a compared step.
  stale_graph(name, mutator): the graph cache is warmed with RolloutDevice(graph=1) on two action buffers (an even and an odd ring) at
      every combination of the tick-slot parity and the done-count parity a handle can be in — a reset launch flips the first alone, a
      step launch both — which is eight graphs, the cache's capacity; then ONE mutator; then RolloutDevice again with the same buffers,
      strides and rings, so that whatever the mutator did to the parities, the old key matches and a graph that was not dropped replays.
  mixed(name, seed): 48 operations drawn from the kinds the configuration accepts, step-like ones about half, with one scripted jump of
      the tick to 2^32 - 3, a share of lanes forced close to termination by every SetState and short time limits, so that tick-keyed
      reset draws matter throughout; every refused call is followed by a step; one scripted run of graph replays around Seed(int) and
      the arrival of per-lane keys."""
import numpy as np

from _handle_replay import CONFIGS, PATHS, STEP_LIKE, accepted, refusals
import _instantiation_matrix as M

MIXED_OPS = 48
MIXED_SEEDS = (0, 1, 2)
TICK_JUMP = 2 ** 32 - 3
KEY_POOL = np.array([0x1234567, 0x9ABCDEF0123, 77, 0x7FFFFFFFFFFFFFF1, 5], dtype=np.int64)


# ---- ingredients -----------------------------------------------------------------------------------------------------------
def actions(c, rng):
    n = c["n"]
    if M.ENVS[c["env"]]["box"]:
        a = rng.uniform(-2.5, 2.5, n).astype(np.float32)
        a[rng.random(n) < 0.05] = -0.0
        return a
    return rng.integers(0, M.ENVS[c["env"]]["nvals"], n).astype(np.int32)


def scalar_action(c, rng):
    return int(rng.integers(-2, 3)) if M.ENVS[c["env"]]["box"] else int(rng.integers(0, M.ENVS[c["env"]]["nvals"]))


def ring_of(c, rng, R):
    return np.stack([actions(c, rng) for _ in range(R)])


def edge_state(c, rng):
    """A float32 start state [S, n] in which a share of the lanes is one to a few steps from termination."""
    n, env = c["n"], c["env"]
    edge = rng.random(n) < c["share"]
    edge[rng.integers(0, n)] = True
    k = int(edge.sum())
    if env.startswith("CartPole"):
        s = rng.uniform(-0.04, 0.04, (4, n))
        side = np.where(rng.random(k) < 0.5, -1.0, 1.0)
        s[:, edge] = np.stack([rng.uniform(-1, 1, k), rng.uniform(-1, 1, k), rng.uniform(0.03, 0.2, k) * side, rng.uniform(1.0, 3.0, k) * side])
    elif env == "Acrobot":
        s = rng.uniform(-0.1, 0.1, (4, n))
        s[:, edge] = np.stack([np.pi - rng.uniform(0, 0.1, k), rng.uniform(-0.1, 0.1, k), rng.uniform(-2, 2, k), rng.uniform(-2, 2, k)])
    else:                                          # Pendulum ends by its time limit alone
        s = np.stack([rng.uniform(-np.pi, np.pi, n), rng.uniform(-8, 8, n)])
    return s.astype(np.float32)


def lengths(c, rng):
    return rng.integers(0, max(c["max_episode_steps"], 6), c["n"]).astype(np.int32)


def lane_keys(c, rng):
    k = KEY_POOL[rng.integers(0, 3, c["n"]) + int(rng.integers(0, 3))]
    k[0], k[-1] = KEY_POOL[0], KEY_POOL[4]          # never all equal
    return k


def lane_mask(c, rng, p=0.3):
    m = (rng.random(c["n"]) < p).astype(np.uint8)
    m[rng.integers(0, c["n"])] = 1
    return m


# ---- operations ------------------------------------------------------------------------------------------------------------
def op_step(c, rng, path=None, st=None):
    if path is None and st is not None:             # a mixed sequence takes the entry points in turn
        path = PATHS["step"][st["steps"] % len(PATHS["step"])]
        st["steps"] += 1
    path = path or PATHS["step"][rng.integers(0, len(PATHS["step"]))]
    return dict(kind="step", path=path, a=scalar_action(c, rng) if path == "StepInt" else actions(c, rng))


def op_rollout(c, rng, path, R, T, fill=True, ring=None):
    return dict(kind="rollout", path=path, buf=f"ring{R}", ring=ring_of(c, rng, R) if ring is None else ring, T=T, fill=fill)


def _graph_T(rng, R):
    """replays of the captured turn (2 for an even ring, 2 * R steps for an odd one) and an eager tail"""
    glen = R if R % 2 == 0 else 2 * R
    return glen * int(rng.integers(1, 3)) + int(rng.integers(0, 2))


def op_random_rollout(c, rng, path=None):
    path = path or PATHS["rollout"][rng.integers(0, 3)]
    R = int(rng.integers(2, 4))
    return op_rollout(c, rng, path, R, _graph_T(rng, R) if path != "fused" else int(rng.integers(3, 6)))


def op_sampled(c, rng):
    return dict(kind="rollout_sampled", T=int(rng.integers(3, 6)), aseed=int(rng.integers(1, 2 ** 40)), atick0=int(rng.integers(0, 2 ** 33)))


def op_eps(c, rng):
    R = int(rng.integers(2, 4))
    return dict(kind="rollout_eps", T=int(rng.integers(3, 6)), eps=float(rng.choice([0.0, 0.25, 0.5, 1.0])), buf=f"ring{R}", ring=ring_of(c, rng, R),
                fill=True, aseed=int(rng.integers(1, 2 ** 40)), atick0=int(rng.integers(0, 2 ** 33)))


def op_decision(c, rng, path=None, R=None):
    return dict(kind="decision", path=path or PATHS["decision"][rng.integers(0, 2)], a=actions(c, rng), R=R or int(rng.choice([1, 3])))


def op_reset(c, rng, path=None):
    return dict(kind="reset", path=path or PATHS["reset"][rng.integers(0, 2)])


def op_reset_where(c, rng, path=None, none=None):
    none = (rng.random() < 0.5) if none is None else none
    return dict(kind="reset_where", path=path or PATHS["reset_where"][rng.integers(0, 2)], mask=None if none else lane_mask(c, rng))


def op_seed(c, rng, form=None):
    form = form or ("int", "keys", "equal")[rng.integers(0, 3)]
    if form == "int":
        return dict(kind="seed", value=int(rng.integers(1, 2 ** 40)))
    if form == "equal":
        return dict(kind="seed", value=np.full(c["n"], int(rng.integers(1, 2 ** 40)), np.int64))
    return dict(kind="seed", value=lane_keys(c, rng))


def op_policy(c, rng, st, field=None):
    """SetLaunchPolicy between the forms the handle accepts; st["vec"] follows the lane width (the misaligned refusal needs it)"""
    fields = ["block", "nt", "graph"] + (["vec"] if c["wide"] else []) + (["reset_form"] if M.ENVS[c["env"]]["alias"] else [])
    f = field or fields[rng.integers(0, len(fields))]
    if f == "vec":
        v = c["wide"] if st["vec"] == 1 else 1
        st["vec"] = v
    else:
        v = int(rng.choice({"block": (64, 128, 256), "nt": (0, 12, 15), "graph": (0, 1, -2), "reset_form": (0, 1)}[f]))
    return dict(kind="noop", what="policy", fields={f: v})


def op_noop(c, rng, st):
    what = ("policy", "policy", "Sync", "GetState", "KernelName", "PackObs")[rng.integers(0, 6)]
    return op_policy(c, rng, st) if what == "policy" else dict(kind="noop", what=what)


def op_refused(c, rng, st, what=None):
    pool = [w for w in refusals(c) if w != "misaligned" or st["vec"] > 1]
    what = what or pool[rng.integers(0, len(pool))]
    op = dict(kind="refused", what=what)
    if what in ("misaligned", "ring0", "epsilon"):
        op.update(buf="ring3", ring=ring_of(c, rng, 3), fill=True)
    if what == "repeat256":
        op["a"] = actions(c, rng)
    if what == "set_sbd":
        op["value"] = np.zeros(c["n"], np.int32)
    if what == "set_array":
        op["value"] = lengths(c, rng)
    return op


def op_of(kind, c, rng, st):
    if kind == "step":
        return op_step(c, rng, st=st)
    if kind in ("rollout", "decision", "reset", "reset_where"):      # the entry points in turn
        st[kind] = st.get(kind, st["first"]) + 1
        path = PATHS[kind][st[kind] % len(PATHS[kind])]
        return {"rollout": op_random_rollout, "decision": op_decision, "reset": op_reset, "reset_where": op_reset_where}[kind](c, rng, path)
    if kind == "rollout_sampled":
        return op_sampled(c, rng)
    if kind == "rollout_eps":
        return op_eps(c, rng)
    if kind == "seed":
        return op_seed(c, rng)
    if kind == "set_lane_seeds":
        return dict(kind=kind, value=lane_keys(c, rng))
    if kind == "set_tick":
        return dict(kind=kind, value=int(rng.integers(0, 2 ** 20)))
    if kind == "set_state":
        return dict(kind=kind, state=edge_state(c, rng))
    if kind == "set_array":
        if rng.random() < 0.6:
            return dict(kind=kind, name="episode_length", value=lengths(c, rng))
        return dict(kind=kind, name="episode_return", value=rng.uniform(-3, 3, c["n"]).astype(np.float32))
    if kind == "set_sbd":
        return dict(kind=kind, value=rng.integers(-1, 3, c["n"]).astype(np.int32))
    if kind == "migrate":
        return dict(kind=kind)
    if kind == "noop":
        return op_noop(c, rng, st)
    raise KeyError(kind)


def _prologue(c, rng):
    ops = [op_reset(c, rng), dict(kind="set_state", state=edge_state(c, rng))]
    if c["episode_stats"]:
        ops.append(dict(kind="set_array", name="episode_length", value=lengths(c, rng)))
    return ops


# ---- mixed sequences ---------------------------------------------------------------------------------------------------------
def mixed(name, seed):
    c = CONFIGS[name]
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    st = dict(vec=(c["launch"] or {}).get("vec", 1), steps=seed, first=seed)      # each rotation of entry points starts at the seed
    acc = accepted(c)
    head = _prologue(c, rng)
    # units: lists of operations that stay together.  One of every accepted kind; the checkpoint / restore pair is ordered below
    units = []
    for kind in sorted(acc - {"checkpoint", "restore", "refused", "step", "seed", "set_lane_seeds"}):
        units.append([kind])
    units += [["refused"], ["checkpoint"], ["restore"], ["jump"], ["set_state"], ["reseed"]]
    ends = [["rollout:graph2"], ["rollout:graph3"]]          # a graph replay before and after everything else
    if not c["auto_reset"]:                         # reset_where(None) must meet set done flags, at least twice
        units += [["own_flags"], ["own_flags"]]
    size = lambda u: {"refused": 2, "jump": 5, "own_flags": 3, "reseed": 6}.get(u[0], 1)      # noqa: E731
    fill = MIXED_OPS - len(head) - len(ends) - sum(size(u) for u in units)
    step_like = [k for k in STEP_LIKE if k in acc]
    others = sorted(acc - set(STEP_LIKE) - {"checkpoint", "restore", "refused", "migrate"})
    for _ in range(fill):
        if rng.random() < 0.8:
            units.append([step_like[rng.choice(len(step_like), p=_weights(step_like))]])
        else:
            units.append([others[rng.integers(0, len(others))]])
    order = rng.permutation(len(units))
    units = [units[i] for i in order]
    ck, rs = units.index(["checkpoint"]), units.index(["restore"])
    if rs < ck:
        units[ck], units[rs] = units[rs], units[ck]
    ops = list(head)
    for u in [ends[0]] + units + [ends[1]]:
        k = u[0]
        if k == "refused":
            ops += [op_refused(c, rng, st), op_step(c, rng, st=st)]
        elif k == "jump":
            ops += [dict(kind="set_tick", value=TICK_JUMP), dict(kind="reset_where", path="ResetWhereDevice", mask=lane_mask(c, rng)),
                    op_step(c, rng, st=st), op_step(c, rng, st=st), dict(kind="reset_where", path="ResetWhere", mask=lane_mask(c, rng))]
        elif k == "reseed":
            # an even number of steps each, so every replay finds the key of the one before: a graph that outlived Seed(int) would draw
            # with the old seed, one that outlived the keys' arrival without them
            ring = ring_of(c, rng, 2)
            ops += [dict(kind="set_state", state=edge_state(c, rng)), op_rollout(c, rng, "graph", 2, 4, ring=ring), op_seed(c, rng, "int"),
                    op_rollout(c, rng, "graph", 2, 4, fill=False, ring=ring), dict(kind="set_lane_seeds", value=lane_keys(c, rng)),
                    op_rollout(c, rng, "graph", 2, 4, fill=False, ring=ring)]
        elif k == "own_flags":
            ops += [dict(kind="set_state", state=edge_state(c, rng)), op_step(c, rng, st=st), op_reset_where(c, rng, none=True)]
        elif k in ("checkpoint", "restore"):
            ops.append(dict(kind=k, slot="m"))
        elif k.startswith("rollout:graph"):
            R = int(k[-1])
            ops.append(op_rollout(c, rng, "graph", R, _graph_T(rng, R)))
        else:
            ops.append(op_of(k, c, rng, st))
    assert len(ops) == MIXED_OPS, len(ops)
    return ops


def _weights(kinds):
    w = np.array([{"step": 4.0, "rollout": 3.0}.get(k, 1.0) for k in kinds])
    return w / w.sum()


# ---- the table, scripted -------------------------------------------------------------------------------------------------------
def policy_forms(c):
    """every SetLaunchPolicy form the handle accepts, as (field, value); the lane width goes to the other form and back"""
    out = [("block", v) for v in (64, 128, 256)] + [("nt", v) for v in (0, 12, 15)] + [("graph", v) for v in (0, 1, -2)]
    if M.ENVS[c["env"]]["alias"]:
        out += [("reset_form", 0), ("reset_form", 1)]
    if c["wide"]:
        first = (c["launch"] or {}).get("vec", 1)
        out += [("vec", c["wide"] if first == 1 else 1), ("vec", first)]
    return out


NOOP_CALLS = ("Sync", "GetState", "KernelName", "PackObs")
SEED_FORMS = ("int", "keys", "equal")


def table(name):
    """Every row of the hand-written table held to the library, nothing drawn: every entry of refusals(c), every policy form, the four
    no-op calls, the three forms of Seed and ResetWhere(None) through both entry points — each followed by a compared step, the entry
    points of the step in turn."""
    c = CONFIGS[name]
    rng = np.random.default_rng([99, sum(map(ord, name))])
    st = dict(vec=(c["launch"] or {}).get("vec", 1), steps=0)
    ops = _prologue(c, rng)

    def then_step(*before):
        ops.extend(before)
        ops.append(op_step(c, rng, st=st))

    for what in refusals(c):
        if what == "misaligned" and st["vec"] == 1:          # the refusal belongs to the wide form
            then_step(op_policy(c, rng, st, "vec"))
        then_step(op_refused(c, rng, st, what))
    for f, v in policy_forms(c):
        if f == "vec":
            st["vec"] = v
        then_step(dict(kind="noop", what="policy", fields={f: v}))
    for what in NOOP_CALLS:
        then_step(dict(kind="noop", what=what))
    for form in SEED_FORMS:
        then_step(op_seed(c, rng, form), dict(kind="set_state", state=edge_state(c, rng)))
    for path in PATHS["reset_where"]:
        then_step(dict(kind="set_state", state=edge_state(c, rng)), op_step(c, rng, st=st), dict(kind="reset_where", path=path, mask=None))
    return ops


# ---- stale-graph scripts -----------------------------------------------------------------------------------------------------
MUTATORS = ("seed_int", "seed_keys", "seed_int_after_keys", "tick", "set_state", "set_array_length", "restore_lane_seeds", "set_lane_seeds",
            "policy_vec", "policy_block", "policy_reset_form", "reset_device", "reset_where_device", "step_repeat_device", "fused_odd",
            "host_step", "content")
# every mutator on A and B (A keeps no episode arrays: SetArray(episode_length) is a refused call there, and the script goes on); D and E
# the subset they accept (Pendulum has no wave-compacted reset form)
STALE = {"A": MUTATORS, "B": MUTATORS, "D": MUTATORS, "E": tuple(m for m in MUTATORS if m != "policy_reset_form")}


def stale_graph(name, mutator):
    c = CONFIGS[name]
    rng = np.random.default_rng([MUTATORS.index(mutator), sum(map(ord, name))])
    st = dict(vec=(c["launch"] or {}).get("vec", 1))
    ops = _prologue(c, rng)
    if mutator == "seed_int_after_keys":
        ops.append(op_seed(c, rng, "keys"))
    if mutator == "restore_lane_seeds":
        ops += [op_seed(c, rng, "keys"), op_step(c, rng, "StepDevice"), dict(kind="checkpoint", slot="keys"), op_seed(c, rng, "int")]
    rings = {2: ring_of(c, rng, 2), 3: ring_of(c, rng, 3)}
    first = True
    for rel in (0, 1):                              # the tick slot against the done-count parity: a reset launch flips the first alone
        for _ in (0, 1):                            # both parities of a step launch
            ops += [op_rollout(c, rng, "graph", 2, 4, fill=first, ring=rings[2]), op_rollout(c, rng, "graph", 3, 6, fill=first, ring=rings[3]),
                    op_step(c, rng, "StepDevice")]
            first = False
        if rel == 0:
            ops.append(dict(kind="reset_where", path="ResetWhereDevice", mask=lane_mask(c, rng)))
    ops.append(dict(kind="set_state", state=edge_state(c, rng)))        # lanes close to termination: the replays below draw resets
    mark = len(ops)
    if mutator == "seed_int":
        ops.append(op_seed(c, rng, "int"))
    elif mutator == "seed_keys":
        ops.append(op_seed(c, rng, "keys"))
    elif mutator == "seed_int_after_keys":
        ops.append(op_seed(c, rng, "int"))
    elif mutator == "tick":
        ops.append(dict(kind="set_tick", value=TICK_JUMP))
    elif mutator == "set_state":
        ops.append(dict(kind="set_state", state=edge_state(c, rng)))
    elif mutator == "set_array_length":
        if c["episode_stats"]:
            ops.append(dict(kind="set_array", name="episode_length", value=lengths(c, rng)))
        else:
            ops.append(op_refused(c, rng, st, "set_array"))
    elif mutator == "restore_lane_seeds":
        ops.append(dict(kind="restore", slot="keys"))
    elif mutator == "set_lane_seeds":
        ops.append(dict(kind="set_lane_seeds", value=lane_keys(c, rng)))
    elif mutator == "policy_vec":
        ops.append(op_policy(c, rng, st, "vec"))
    elif mutator == "policy_block":
        ops.append(dict(kind="noop", what="policy", fields={"block": 64}))
    elif mutator == "policy_reset_form":
        ops.append(dict(kind="noop", what="policy", fields={"reset_form": 0 if (c["launch"] or {}).get("reset_form") == 1 else 1}))
    elif mutator == "reset_device":
        ops.append(op_reset(c, rng, "ResetDevice"))
    elif mutator == "reset_where_device":
        ops.append(dict(kind="reset_where", path="ResetWhereDevice", mask=lane_mask(c, rng)))
    elif mutator == "step_repeat_device":
        ops.append(op_decision(c, rng, "StepRepeatDevice", 3))
    elif mutator == "fused_odd":
        ops.append(op_rollout(c, rng, "fused", 3, 5, fill=False, ring=rings[3]))
    elif mutator == "host_step":
        ops.append(op_step(c, rng, "Step"))
    elif mutator == "content":
        rings = {2: ring_of(c, rng, 2), 3: ring_of(c, rng, 3)}
    else:
        raise KeyError(mutator)
    changed = mutator == "content"
    if mutator == "reset_device":
        ops.append(dict(kind="set_state", state=edge_state(c, rng)))    # (a reset leaves no lane close to termination)
    ops += [op_rollout(c, rng, "graph", 2, 5, fill=changed, ring=rings[2]), op_rollout(c, rng, "graph", 3, 6, fill=changed, ring=rings[3]),
            op_step(c, rng, "StepDevice"), op_rollout(c, rng, "graph", 2, 4, fill=False, ring=rings[2])]
    return ops, mark
