"""The call sequences of tests/_call_sequences.py, run on the model alone (tests/_handle_replay.py HandleModel): what they cover is
asserted here, so tests/test_gpu_call_sequences.py compares a handle with sequences that are known to reach the edges — and the model
is held to the oracle: a rollout is its steps, a restored checkpoint continues as the original did, lanes do not depend on the batch
they are stepped in."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _call_sequences as Q  # noqa: E402
import _handle_replay as H  # noqa: E402

NAMES = sorted(H.CONFIGS)
MUTATOR_KINDS = ("seed", "set_lane_seeds", "set_tick", "set_state", "set_array", "set_sbd", "restore", "migrate", "reset", "reset_where",
                 "decision", "rollout_sampled", "rollout_eps", "noop")


def _same(sa, sb):
    for k in sa:
        if sa[k] is None or sb[k] is None:
            if not (sa[k] is None and sb[k] is None):
                return False
        elif isinstance(sa[k], np.ndarray):
            if H.first_diff(sa[k], sb[k]) is not None:
                return False
        elif sa[k] != sb[k]:
            return False
    return True


def run(oracle, name, ops):
    """The sequence on a model; per operation: its kind, whether a step-like one finished a lane, the ticks of its reset draws, the set
    done flags a reset_where(None) met, a fingerprint of the model afterwards."""
    m = H.HandleModel(oracle, H.CONFIGS[name])
    slots, trace = {}, []
    for op in ops:
        d0 = len(m.draw_ticks)
        met = int((m.done != 0).sum()) if (op["kind"] == "reset_where" and op["mask"] is None) else None
        before = m.snapshot()
        rec = H.apply(m, op, slots)
        recs = rec if isinstance(rec, list) else ([rec] if isinstance(rec, dict) else [])
        after = m.snapshot()
        same = _same(before, after)
        trace.append(dict(kind=op["kind"], path=op.get("path"), finished=any(len(r["lanes"]) for r in recs), draws=m.draw_ticks[d0:], met=met,
                          unchanged=same))
    return m, trace


@pytest.fixture(scope="module")
def traces(oracle):
    return {(name, seed): run(oracle, name, Q.mixed(name, seed))[1] for name in NAMES for seed in Q.MIXED_SEEDS}


@pytest.mark.parametrize("name", NAMES)
def test_mixed_sequences_hold_every_accepted_kind_and_step_about_half_the_time(traces, name):
    for seed in Q.MIXED_SEEDS:
        tr = traces[(name, seed)]
        assert len(tr) == Q.MIXED_OPS
        assert {t["kind"] for t in tr} == H.accepted(H.CONFIGS[name]), (seed, H.accepted(H.CONFIGS[name]) - {t["kind"] for t in tr})
        share = sum(t["kind"] in H.STEP_LIKE for t in tr) / len(tr)
        assert 0.4 <= share <= 0.65, (seed, share)


@pytest.mark.parametrize("name", NAMES)
def test_a_graph_replay_stands_on_both_sides_of_every_kind_of_mutator(traces, name):
    missing = set(MUTATOR_KINDS) & H.accepted(H.CONFIGS[name])
    for seed in Q.MIXED_SEEDS:
        tr = traces[(name, seed)]
        graph = [i for i, t in enumerate(tr) if t["kind"] == "rollout" and t["path"] == "graph"]
        for i, t in enumerate(tr):
            if t["kind"] in missing and graph and graph[0] < i < graph[-1]:
                missing.discard(t["kind"])
    assert not missing, missing
    # every entry point of a kind that has several is taken somewhere in the configuration's three sequences
    for kind, paths in H.PATHS.items():
        taken = {t["path"] for seed in Q.MIXED_SEEDS for t in traces[(name, seed)] if t["kind"] == kind}
        assert taken == set(paths), (kind, set(paths) - taken)


@pytest.mark.parametrize("name", NAMES)
def test_a_quarter_of_the_step_like_operations_finish_a_lane(traces, name):
    for seed in Q.MIXED_SEEDS:
        steps = [t for t in traces[(name, seed)] if t["kind"] in H.STEP_LIKE]
        assert sum(t["finished"] for t in steps) * 4 >= len(steps), (seed, sum(t["finished"] for t in steps), len(steps))


@pytest.mark.parametrize("name", [n for n in NAMES if not H.CONFIGS[n]["auto_reset"]])
def test_reset_where_none_meets_set_done_flags(traces, name):
    for seed in Q.MIXED_SEEDS:
        met = [t["met"] for t in traces[(name, seed)] if t["met"]]
        assert len(met) >= 2, (seed, met)


@pytest.mark.parametrize("name", NAMES)
def test_draws_fall_on_both_sides_of_the_low_tick_word(traces, name):
    both = 0
    for seed in Q.MIXED_SEEDS:
        draws = [d for t in traces[(name, seed)] for d in t["draws"]]
        both += any(d < 2 ** 32 for d in draws) and any(d >= 2 ** 32 for d in draws)
        assert any(2 ** 32 - 3 <= d < 2 ** 32 for d in draws) and any(2 ** 32 <= d < 2 ** 32 + 64 for d in draws), seed    # the scripted jump
    assert both >= 1


@pytest.mark.parametrize("name", NAMES)
def test_every_refused_call_leaves_the_model_alone_and_is_followed_by_a_step(traces, name):
    seen = 0
    for seed in Q.MIXED_SEEDS:
        tr = traces[(name, seed)]
        for i, t in enumerate(tr):
            if t["kind"] == "refused":
                seen += 1
                assert t["unchanged"] and tr[i + 1]["kind"] == "step", (seed, i)
            if t["kind"] == "noop":
                assert t["unchanged"], (seed, i)
    assert seen >= 3


@pytest.mark.parametrize("name", sorted(Q.STALE))
def test_stale_graph_scripts_replay_on_both_sides_of_the_mutator_and_draw_resets_after_it(oracle, name):
    for mut in Q.STALE[name]:
        ops, mark = Q.stale_graph(name, mut)
        _, tr = run(oracle, name, ops)
        graph = [i for i, t in enumerate(tr) if t["kind"] == "rollout" and t["path"] == "graph"]
        assert len([i for i in graph if i < mark]) == 8 and len([i for i in graph if i >= mark]) == 3, mut
        # the replays after the mutator make reset draws: a graph that froze the old seed, keys or buffers would show
        assert any(tr[i]["draws"] for i in graph if i >= mark), mut
        for R in (2, 3):                             # the same buffer, stride and ring on both sides
            assert {op["buf"] for op in ops if op["kind"] == "rollout" and len(op["ring"]) == R} == {f"ring{R}"}


@pytest.mark.parametrize("name", NAMES)
def test_the_table_script_holds_every_row_each_followed_by_a_step(oracle, name):
    c = H.CONFIGS[name]
    ops = Q.table(name)
    _, tr = run(oracle, name, ops)

    def followed(i):                                 # by a step, directly or behind the SetState that puts lanes close to termination
        rest = [op["kind"] for op in ops[i + 1:i + 3]]
        return rest[:1] == ["step"] or rest == ["set_state", "step"]

    refused = [op["what"] for op in ops if op["kind"] == "refused"]
    assert sorted(refused) == sorted(H.refusals(c)) and len(refused) >= 5, refused
    policies = [next(iter(op["fields"].items())) for op in ops if op["kind"] == "noop" and op["what"] == "policy"]
    assert set(Q.policy_forms(c)) <= set(policies), set(Q.policy_forms(c)) - set(policies)
    assert {("graph", -2), ("graph", 0), ("graph", 1), ("nt", 0), ("nt", 12), ("nt", 15), ("block", 64), ("block", 128), ("block", 256)} <= set(policies)
    if c["wide"]:
        assert {("vec", 1), ("vec", c["wide"])} <= set(policies)
    assert {op["what"] for op in ops if op["kind"] == "noop"} == {"policy"} | set(Q.NOOP_CALLS)
    seeds = [op["value"] for op in ops if op["kind"] == "seed"]
    assert sum(np.ndim(v) == 0 for v in seeds) == 1                                             # Seed(int)
    assert sum(np.ndim(v) == 1 and (v == v[0]).all() for v in seeds) == 1                        # an all-equal key vector
    assert sum(np.ndim(v) == 1 and not (v == v[0]).all() for v in seeds) == 1                    # per-lane keys
    none = [(i, op["path"]) for i, op in enumerate(ops) if op["kind"] == "reset_where" and op["mask"] is None]
    assert {p for _, p in none} == set(H.PATHS["reset_where"])
    for i, _ in none:
        if c["auto_reset"]:
            assert tr[i]["unchanged"], i              # a no-op that moves no tick
        else:
            assert tr[i]["met"] > 0, i
    for i, op in enumerate(ops):
        if op["kind"] in ("refused", "noop", "seed") or (op["kind"] == "reset_where" and op["mask"] is None):
            assert followed(i), (i, op["kind"])
        if op["kind"] in ("refused", "noop"):
            assert tr[i]["unchanged"], i
        if op["kind"] == "refused" and op["what"] == "misaligned":
            assert any(o["kind"] == "noop" and o.get("fields") == {"vec": c["wide"]} for o in ops[:i]) or (c["launch"] or {}).get("vec", 1) == c["wide"]
    assert {op["path"] for op in ops if op["kind"] == "step"} == set(H.PATHS["step"])


# ---- the model against the oracle ------------------------------------------------------------------------------------------
def _eq_models(a, b):
    sa, sb = a.snapshot(), b.snapshot()
    for k in sa:
        if k == "lane_steps":
            continue
        if sa[k] is None or sb[k] is None:
            assert sa[k] is None and sb[k] is None, k
        elif isinstance(sa[k], np.ndarray):
            assert H.first_diff(sa[k], sb[k]) is None, (k, H.first_diff(sa[k], sb[k]))
        else:
            assert sa[k] == sb[k], k


@pytest.mark.parametrize("name", NAMES)
def test_a_rollout_is_its_steps(oracle, name):
    c = H.CONFIGS[name]
    rng = np.random.default_rng(5)
    a, b = H.HandleModel(oracle, c), H.HandleModel(oracle, c)
    ring = Q.ring_of(c, rng, 3)
    for m in (a, b):
        for op in Q._prologue(c, np.random.default_rng(6)):
            H.apply(m, op, {})
    recs = a.rollout(ring, 7)
    for t in range(7):
        r = b.step(ring[t % 3])
        assert H.first_diff(r["obs"], recs[t]["obs"]) is None and H.first_diff(r["done"], recs[t]["done"]) is None
    _eq_models(a, b)
    assert a.tick == b.tick == 8 and a.lane_steps == 7 * c["n"]
    # a decision of one sub-step is a step
    act = Q.actions(c, rng)
    a.decision(act, 1)
    b.step(act)
    _eq_models(a, b)


@pytest.mark.parametrize("name", NAMES)
def test_a_restored_checkpoint_continues_as_the_original_did(oracle, name):
    ops = Q.mixed(name, 1)
    k = len(ops) // 2
    a = H.HandleModel(oracle, H.CONFIGS[name])
    slots = {}
    for op in ops[:k]:
        H.apply(a, op, slots)
    ck = a.checkpoint()
    b = H.HandleModel(oracle, H.CONFIGS[name])
    b.restore(ck)
    sb = dict(slots)
    tail = [op for op in ops[k:] if op["kind"] not in ("restore",)]
    for op in tail:
        ra, rb = H.apply(a, op, slots), H.apply(b, op, sb)
        if isinstance(ra, dict):
            assert H.first_diff(ra["obs"], rb["obs"]) is None and H.first_diff(ra["reward"], rb["reward"]) is None
    _eq_models(a, b)


@pytest.mark.parametrize("name", ["B", "C", "D", "E", "F"])
def test_split_lanes_equal_the_whole_batch(oracle, name):
    c = H.CONFIGS[name]
    n, k = c["n"], 130
    rng = np.random.default_rng(9)
    whole = H.HandleModel(oracle, c)
    parts = [H.HandleModel(oracle, c, n=k), H.HandleModel(oracle, c, n=n - k, lane_offset=c["lane_offset"] + k)]
    cut = [slice(0, k), slice(k, n)]
    s0, ln0, mask = Q.edge_state(c, rng), Q.lengths(c, rng), Q.lane_mask(c, rng)
    for m, sl in zip([whole] + parts, [slice(0, n)] + cut):
        m.reset()
        m.set_state(s0[:, sl])
        m.set_array("episode_length", ln0[sl])
    for t in range(6):
        a = Q.actions(c, rng)
        for m, sl in zip([whole] + parts, [slice(0, n)] + cut):
            m.step(a[sl]) if t % 3 else m.decision(a[sl], 3)
            if t == 3:
                m.reset_where(mask[sl])
    for m in [whole] + parts:
        m.rollout_sampled(4, 77, 2 ** 32 - 2)
    for key in ("s", "obs", "reward", "done", "ret", "ln", "fin_ret", "fin_len"):
        got = np.concatenate([getattr(p, key) for p in parts], axis=-1)
        assert H.first_diff(got, getattr(whole, key)) is None, key
    assert whole.tick == parts[0].tick == parts[1].tick
