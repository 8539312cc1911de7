"""CPU checks of the adversarial episode-memory scripts (tests/_episode_memory_cases.py): what they must cover, stated on the model's
trace of each script, and the model's top-K-per-push form held to the sequential EndEpisode rule on every one of them.  The GPU test
(tests/test_gpu_episode_memory_keys.py) runs the same scripts, so a script that stopped covering its case fails here, without a GPU."""
import functools

import numpy as np
import pytest

import _episode_memory_cases as cases
import _episode_memory_model as model


@functools.lru_cache(maxsize=None)
def _traced():
    return [(s, cases.model_trace(s)[1]) for s in cases.scripts()]


def _of(family):
    got = [(s, tr) for s, tr in _traced() if s["family"] == family]
    assert got, family
    return got


def _valid(rec):
    return [e for e in rec["ended"] if not model.is_nan(e["ret"])]


def _evicts(rec):
    after = {id(e) for e in rec["pool"]}
    return any(id(e) not in after for e in rec["before"])


def _admits_on_equal_return(rec, capacity):
    if len(rec["before"]) < capacity:
        return False
    thr = min(float(e["ret"]) for e in rec["before"])
    after = {id(e) for e in rec["pool"]}
    return any(float(e["ret"]) == thr and id(e) in after for e in _valid(rec))


def test_every_family_is_present_and_names_are_unique():
    assert {s["family"] for s, _ in _traced()} == set(cases.FAMILIES)
    names = [s["name"] for s, _ in _traced()]
    assert len(names) == len(set(names))
    for s, _ in _traced():
        assert s["env"] in ("CartPole-v1", "Pendulum-v1") and s["dtype"] in ("float32", "float64")
        for seg in s["segments"]:
            assert seg["reward"].dtype == np.uint32 and seg["done"].dtype == np.uint8 and seg["reward"].shape == seg["done"].shape
            assert seg["reward"].shape[1] == s["n"] and seg["reward"].shape[0] <= 64
    assert any(s["dtype"] == "float64" for s, _ in _traced()) and any(s["env"] == "Pendulum-v1" for s, _ in _traced())
    assert {s["n"] for s, _ in _traced()} >= {64, 257, 1027}


def test_every_digit_decides_a_selection():
    """Every digit of the key decides the selection of at least one push.  Digit 12, the lane's top byte, cannot in a script of ordinary
    size: two lanes differ there only when they are 2^24 apart (cases.LANE_TOP_BYTE, which the GPU test runs on its own)."""
    decided = {}
    for s, tr in _traced():
        for rec in tr:
            d = cases.deciding_digit(rec["before"], rec["ended"], s["capacity"])
            if d is not None:
                decided.setdefault(d, s["name"])
    assert set(decided) == set(range(16)) - {12}, decided
    c = cases.LANE_TOP_BYTE
    ended = [{"ret": np.float32(c["ret"]), "len": c["steps"], "tick": cases.TICK0 + c["steps"], "lane": lane} for lane in c["lanes"]]
    assert max(c["lanes"]) < c["n"] and cases.deciding_digit([], ended, c["capacity"]) == 12
    assert model.top_k_per_push([], ended, 1) == [ended[1]]
    assert model.end_episode_sequential(model.end_episode_sequential([], ended[0], 1), ended[1], 1) == [ended[1]]


def test_every_family_evicts_and_admits_on_an_equal_return():
    for family in cases.FAMILIES:
        recs = [(s, rec) for s, tr in _of(family) for rec in tr]
        assert any(_evicts(rec) for _, rec in recs), family
    for family in ("sign_fold", "ties", "nan", "capacity", "stale", "equal_keys"):
        assert any(_admits_on_equal_return(rec, s["capacity"]) for s, tr in _of(family) for rec in tr), family


def test_sign_fold_holds_every_value_in_one_pool_and_the_boundary_between_every_pair():
    s, tr = next((s, tr) for s, tr in _of("sign_fold") if s["name"] == "fold_all")
    folded = sorted({model.ret_bits(cases.as_float(b)) for b in cases.FOLD})
    assert len(folded) == 15                                               # the two zeros are one return
    assert any(sorted({model.ret_bits(e["ret"]) for e in rec["pool"]}) == folded for rec in tr)
    lowest_kept = [min(model.ret_bits(e["ret"]) for e in rec["pool"]) for rec in tr if _evicts(rec)]
    assert set(folded[1:]) <= set(lowest_kept)                             # every value was the lowest kept right after its lower neighbour left
    s, tr = next((s, tr) for s, tr in _of("sign_fold") if s["name"] == "fold_up")
    assert tr[-1]["stats"]["admitted"] == len(cases.FOLD)
    s, tr = next((s, tr) for s, tr in _of("sign_fold") if s["name"] == "fold_down")
    assert tr[-1]["stats"] == dict(kept=2, ended=16, admitted=2, too_long=0)


def test_nan_family_meets_every_pool_state():
    for s, tr in _of("nan"):
        k, states, kinds, places = s["capacity"], set(), set(), set()
        seg = s["segments"][0]
        for rec in tr:
            nans = [e for e in rec["ended"] if model.is_nan(e["ret"])]
            if not nans:
                continue
            fill = len(rec["before"])
            states.add("empty" if fill == 0 else "full" if fill == k else "half")
            if len(nans) == 1 and len(rec["ended"]) == 1:
                states.add("alone")
            if fill == k and len(nans) == len(rec["ended"]):
                states.add("full, NaN only")
            for e in nans:                                                 # where in the episode the NaN arises, and from what
                t_end = rec["step"]
                rew = seg["reward"][t_end - e["len"] + 1:t_end + 1, e["lane"]]
                run, first = np.float32(0), None                           # the step at which the running sum turns NaN
                with np.errstate(invalid="ignore"):
                    for i, b in enumerate(rew):
                        run = np.float32(run + cases.as_float(b))
                        if first is None and np.isnan(run):
                            first = i
                kind = next(name for name, v in cases.NANS.items()
                            if int(rew[first]) == v[-1] and (len(v) == 1 or int(rew[first - 1]) == v[0]))
                kinds.add(kind)
                start = first - (len(cases.NANS[kind]) - 1)
                places.add("first" if start == 0 else "last" if first == e["len"] - 1 else "middle")
        assert states == {"empty", "half", "full", "alone", "full, NaN only"}, states
        assert kinds == set(cases.NANS), kinds
        assert places == {"first", "middle", "last"}, places
        # ordinary episodes are admitted after each of them, and the pool never holds a NaN
        last_nan = max(i for i, rec in enumerate(tr) if any(model.is_nan(e["ret"]) for e in rec["ended"]))
        assert tr[-1]["stats"]["admitted"] > tr[last_nan]["stats"]["admitted"]
        first_nan = min(i for i, rec in enumerate(tr) if any(model.is_nan(e["ret"]) for e in rec["ended"]))
        assert len(tr[first_nan]["before"]) == 0 and tr[-1]["stats"]["kept"] == k
        assert all(not model.is_nan(e["ret"]) for rec in tr for e in rec["pool"])


def test_capacity_family_meets_every_edge():
    by = {s["name"]: (s, tr) for s, tr in _of("capacity")}
    assert by["cap_k1"][0]["capacity"] == 1
    s, tr = by["cap_total"]
    totals = [len(rec["before"]) + len(_valid(rec)) - s["capacity"] for rec in tr]
    assert totals[:3] == [-2, 0, 1] and max(len(_valid(rec)) for rec in tr) > s["capacity"]
    s, tr = by["cap_burst"]
    assert all(len(rec["ended"]) in (0, s["n"]) for rec in tr) and s["n"] > s["capacity"]
    s, tr = by["cap_l1"]
    assert s["max_length"] == 1 and all(len(rec["ended"]) == s["n"] for rec in tr)
    s, tr = by["cap_l2"]
    assert {e["len"] for e in tr[-1]["pool"]} == {1, 2} and tr[-1]["stats"]["too_long"] == 0
    s, tr = by["cap_len"]
    assert tr[-1]["stats"]["too_long"] == 3 and max(e["len"] for e in tr[-1]["pool"]) == s["max_length"]
    s, tr = _of("large_k")[0]
    assert len(tr[1]["ended"]) > s["capacity"] and len(tr[1]["pool"]) == s["capacity"]
    evicted = sum(1 for e in tr[1]["pool"] if id(e) not in {id(x) for x in tr[3]["pool"]})
    assert 0.3 * s["capacity"] < evicted < 0.7 * s["capacity"]
    for k, n in ((65536, 66001), (16384, 66001)):                          # the sizes the GPU test builds
        big = cases.large_k(k, n, "big")
        assert big["n"] >= 66000 and big["max_length"] <= 4 and int(big["segments"][0]["done"][1].sum()) > 65536


@pytest.mark.parametrize("chunk", [3, 16])
def test_stale_family_fills_the_pool_inside_a_pass(chunk):
    for s, tr in _of("stale"):
        k = s["capacity"]
        assert chunk in s["chunks"] and len(tr) % chunk != 0
        found = False
        for t0 in range(0, len(tr), chunk):
            rows = tr[t0:t0 + chunk]
            if len(rows[0]["before"]) >= k:
                continue
            fills = next((j for j, rec in enumerate(rows) if len(rec["pool"]) == k), None)
            if fills is None:
                continue
            below = equal = nan = none_counts = False
            for rec in rows[fills + 1:]:                                   # every ender here passes the scan's stale filter
                thr = min(float(e["ret"]) for e in rec["before"])
                rets = [float(e["ret"]) for e in _valid(rec)]
                below |= any(r < thr for r in rets)
                equal |= any(r == thr for r in rets)
                nan |= len(_valid(rec)) < len(rec["ended"])
                none_counts |= bool(rec["ended"]) and all(r < thr for r in rets)
            found |= below and equal and nan and none_counts
        assert found, (s["name"], chunk)


def test_equal_keys_family_holds_duplicates_at_the_selection():
    for s, tr in _of("equal_keys"):
        k = s["capacity"]
        keys = [model.key(e) for e in tr[-1]["pool"]]
        assert len(set(keys)) < len(keys)                                  # the pool ends with equal keys in it
        split = pool_pair = False
        for rec in tr:
            every = sorted(rec["before"] + _valid(rec), key=model.key, reverse=True)
            if len(every) > k and model.key(every[k - 1]) == model.key(every[k]):
                split = True                                               # the K-th key has an equal below it
                pool_pair |= sum(1 for e in rec["before"] if model.key(e) == model.key(every[k])) >= 2
        assert split and pool_pair, s["name"]                              # ... once with both equals already in the pool
        if s["equal_keys"] == "backwards":                                 # different markers (different rows) under one key
            assert len({v[:3] for v in s["markers"].values()}) < len(s["markers"])


@pytest.mark.parametrize("name", [s["name"] for s in cases.scripts()])
def test_top_k_per_push_equals_the_sequential_rule_on_every_script(name):
    s, tr = next((s, tr) for s, tr in _traced() if s["name"] == name)
    pool = []
    for rec in tr:
        for e in sorted(rec["ended"], key=lambda e: (e["tick"], e["lane"])):
            pool = model.end_episode_sequential(pool, e, s["capacity"])
        assert sorted(map(model.key, pool)) == sorted(map(model.key, rec["pool"])), (name, rec["segment"], rec["step"])
        assert {id(e) for e in pool} == {id(e) for e in rec["pool"]}, (name, rec["segment"], rec["step"])
    assert tr[-1]["stats"]["ended"] > 0
