"""The edge-state tables of Pendulum, MountainCar and Acrobot (tests/_env_edge_tables.py) against both oracles, on the CPU: every
branch of each step is taken by some row, the hand-derived facts hold in the float64 statement of upstream AND in the float32
kernel-semantics twin, the twin stays within the GPU tests' bars of float64 on every finite row — and the proof that the Acrobot
kernel's shortcuts (a bounded wrap, a small-argument sin / cos) hold on the env's own closed state box."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _env_edge_tables as T  # noqa: E402

f32 = np.float32
ENVS = ("Pendulum-v1", "MountainCar-v0", "Acrobot-v1")

# What envs.hpp and docs/ledger.md state; the domain test measures both again and fails if they stop being true.
DOCUMENTED_PRE_WRAP_MAX = 29.73           # rad, the largest |angle| before the wrap over the closed state box (measured 29.724)
DOCUMENTED_STAGE_MAX = 33.32              # rad, the largest |angle| an RK4 stage hands to sin / cos (measured 33.317)


def run_table(oracle, env, dtype):
    """One step of the env's table in one oracle: dict(rows, s, a, s2, obs, reward, done[, wraps])."""
    rows, s, a = T.table_arrays(env)
    out = dict(rows=rows, s=s, a=a)
    if env == "Pendulum-v1":
        out["s2"], out["obs"], out["reward"], out["done"] = oracle.pendulum_step(s, a, dtype=dtype)
    elif env == "MountainCar-v0":
        out["s2"], out["reward"], out["done"] = oracle.mountaincar_step(s, a, dtype=dtype)
        out["obs"] = out["s2"]
    else:
        out["s2"], out["obs"], out["reward"], out["done"] = oracle.acrobot_step(s, a, dtype=dtype)
        p = oracle.acrobot_domain_probe(s, a)
        out["wraps"] = p["wraps64"] if dtype == np.float64 else p["wrapsk"]
        assert np.array_equal(out["s2"], p["next64"] if dtype == np.float64 else p["nextk"], equal_nan=True)     # the probe IS the step
        out["literal"] = p["nextlit"]
    return out


@pytest.fixture(scope="module")
def stepped(oracle):
    return {(env, dt): run_table(oracle, env, dt) for env in ENVS for dt in (np.float64, f32)}


# ---- the tables themselves ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ENVS)
def test_tables_are_deterministic_and_hold_what_the_issue_lists(env):
    rows, s, a = T.table_arrays(env)
    rows2, s2, a2 = T.table_arrays(env)
    assert [r["name"] for r in rows] == [r["name"] for r in rows2]
    assert np.array_equal(s, s2, equal_nan=True) and np.array_equal(a, a2, equal_nan=True)
    assert s.dtype == f32 and s.shape == (T.STATE_DIM[env], len(rows))
    assert any(not r["finite"] for r in rows) and all(r["facts"] for r in rows)
    # NaN and +-inf in each state component
    for c in range(s.shape[0]):
        col = s[c]
        assert np.isnan(col).any() and (col == np.inf).any() and (col == -np.inf).any(), (env, c)
    if env == "Acrobot-v1":
        for c, m in ((2, T.MV1), (3, T.MV2)):
            assert (s[c] == m).any() and (s[c] == -m).any()
        assert (np.abs(s[:2]) == T.PI32).any()
    if env == "Pendulum-v1":
        assert np.isnan(a).any() and (a == np.inf).any() and (a == -np.inf).any() and np.signbit(a[a == 0]).any()
        assert (np.abs(s[0]) > 65536).any() and (np.abs(s[0]) >= f32(4194304.0) * T.TWO_PI32).any()
    if env == "MountainCar-v0":
        assert {-1, 3, 7} <= set(a.tolist())


# ---- branch coverage -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, f32], ids=["float64", "twin"])
@pytest.mark.parametrize("env", ENVS)
def test_every_branch_of_the_step_is_taken_by_some_row(stepped, env, dtype):
    t = stepped[(env, dtype)]
    if env == "Pendulum-v1":
        per_row, want = T.pendulum_branches(t["s"], t["a"], t["s2"], dtype), T.PENDULUM_BRANCHES
    elif env == "MountainCar-v0":
        per_row, want = T.mountaincar_branches(t["s"], t["a"], t["s2"], t["done"], dtype), T.MOUNTAINCAR_BRANCHES
    else:
        use = np.array([r["upstream"] for r in t["rows"]])
        per_row = [b if u else set() for b, u in zip(T.acrobot_branches(t["s2"], t["done"], t["wraps"], dtype), use)]
        want = T.ACROBOT_BRANCHES
    taken = set().union(*per_row)
    assert want <= taken, sorted(want - taken)


# ---- hand facts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, f32], ids=["float64", "twin"])
@pytest.mark.parametrize("env", ENVS)
def test_hand_derived_facts_hold(stepped, env, dtype):
    t = stepped[(env, dtype)]
    T.check_facts(t["rows"], t["s2"], t["reward"], t["done"], dtype, "f64" if dtype == np.float64 else "twin")


# ---- twin against float64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ENVS)
def test_twin_stays_within_the_bars_of_float64_on_every_finite_row(stepped, env):
    """Integer outputs equal on every row, states within the bars tests/test_gpu_other_envs.py uses (T.check_float64_bars)."""
    a, b = stepped[(env, np.float64)], stepped[(env, f32)]
    use = np.array([r["upstream"] for r in a["rows"]])
    assert use.sum() >= np.array([r["finite"] for r in a["rows"]]).sum() - 8          # (only rows far outside Acrobot's bounds are left out)
    T.check_float64_bars(env, a["s"], a, b, use, literal=b.get("literal"))


def test_no_acrobot_row_lies_in_the_termination_exemption_band(stepped):
    """tests/test_gpu_other_envs.py exempts lanes whose float64 height is within 1e-4 of the termination threshold.  No row of the
    table is there, so nothing is exempted here; the termination rows are at least 1e-3 away, on their stated side."""
    a = stepped[("Acrobot-v1", np.float64)]
    use = np.array([r["upstream"] for r in a["rows"]])
    want = a["s2"]
    height = -np.cos(want[0]) - np.cos(want[0] + want[1])
    assert np.abs(height[use] - 1.0).min() >= 1e-4
    named = {r["name"]: i for i, r in enumerate(a["rows"])}
    for name, _, _, d in T.ACROBOT_TERMINATION:
        h = height[named[name]]
        assert (h - 1.0 >= 1e-3) if d else (1.0 - h >= 1e-3), (name, h)
    assert a["done"][use].any() and not a["done"][use].all()


# ---- the Acrobot domain proof ----------------------------------------------------------------------------------------------------
BOUNDARY_BAND = 1e-3      # rad: a pre-wrap angle this close to an odd multiple of pi may wrap once more / less in float32 (same point on the circle)


@pytest.fixture(scope="module")
def search(oracle):
    k = oracle.acrobot_wrap_k()
    acc = dict(n=0, over4=0, max_wraps=0, count_mismatch=0, count_far=0, done_mismatch=0, outside=0,
               dang=0.0, dvel=0.0, lang=0.0, lvel=0.0, sum_dang=0.0, sum_lang=0.0, stage_twin=0.0, pinned=0)

    def visit(s, a, o):
        acc["n"] += s.shape[1]
        acc["pinned"] += int(((np.abs(s[2]) == T.MV1) | (np.abs(s[3]) == T.MV2)).sum())
        w64, wk = o["wraps64"], o["wrapsk"]
        acc["max_wraps"] = max(acc["max_wraps"], int(w64.max()))
        acc["over4"] += int((w64.max(0) > 4).sum())
        m = np.abs(o["pre64"][:2])
        d = np.mod(m - np.pi, 2.0 * np.pi)
        near = np.minimum(d, 2.0 * np.pi - d) < BOUNDARY_BAND
        diff = np.abs(w64 - wk)
        acc["count_mismatch"] += int((diff[~near] != 0).sum())
        acc["count_far"] += int((diff > 1).sum())
        acc["outside"] += int((np.abs(o["nextk"][:2]) > T.PI32).sum())
        dang, dvel = T.acrobot_errors(o["nextk"], o["next64"])
        lang, lvel = T.acrobot_errors(o["nextlit"], o["next64"])
        for key, v in (("dang", dang), ("dvel", dvel), ("lang", lang), ("lvel", lvel)):
            acc[key] = max(acc[key], float(v.max()))
        acc["sum_dang"] += float(dang.sum()); acc["sum_lang"] += float(lang.sum())
        acc["stage_twin"] = max(acc["stage_twin"], float(o["prek"][2].max()))
        h = -np.cos(o["next64"][0]) - np.cos(o["next64"][0] + o["next64"][1])
        acc["done_mismatch"] += int(((o["done64"] != o["donek"]) & (np.abs(h - 1.0) >= 1e-4)).sum())

    best = T.acrobot_search(oracle, visit)
    return dict(acc, k=k, pre=best["pre"], stage=best["stage"])


def test_acrobot_search_covers_what_the_issue_asks(search):
    assert search["n"] >= (1 << 24) + 243
    assert search["pinned"] >= (1 << 24) // 4


def test_acrobot_wrap_covers_the_measured_pre_wrap_maximum_plus_a_turn(search):
    pre, k = search["pre"][0], search["k"]
    print(f"pre-wrap maximum {pre:.4f} rad at {search['pre'][1:]}, k = {k} covers {(2 * k + 1) * np.pi:.4f}")
    assert search["max_wraps"] == 5 and search["over4"] > 0                    # four subtractions (9 pi = 28.27) do NOT cover the box
    assert pre > 9 * np.pi
    assert pre + 2.0 * np.pi <= (2 * k + 1) * np.pi                             # the measured maximum plus one full turn
    assert pre + 2.0 * np.pi > (2 * (k - 1) + 1) * np.pi                        # ... and k - 1 would not do
    assert DOCUMENTED_PRE_WRAP_MAX - 0.05 <= pre <= DOCUMENTED_PRE_WRAP_MAX     # what envs.hpp and docs/ledger.md state


def test_sincos_small_is_swept_as_far_as_the_stages_reach(search):
    stage = search["stage"][0]
    print(f"stage maximum {stage:.4f} rad at {search['stage'][1:]} (twin {search['stage_twin']:.4f}); sweep to {T.SINCOS_SMALL_SWEEP}")
    assert stage > 24.0                                                         # beyond what the function was documented for
    # (tests/test_oracle.py sweeps sincos_small to T.SINCOS_SMALL_SWEEP)
    assert T.SINCOS_SMALL_SWEEP >= stage + np.pi and T.SINCOS_SMALL_SWEEP >= search["stage_twin"] + np.pi
    assert DOCUMENTED_STAGE_MAX - 0.05 <= stage <= DOCUMENTED_STAGE_MAX


def test_bounded_wrap_equals_the_unbounded_loop_on_every_searched_state(search):
    """The twin with k subtractions against the float64 oracle's unbounded loop: the same number of wraps (an angle within 1e-3 rad
    of an odd multiple of pi before the wrap may take one more or one less in float32 — the same point on the circle), every stored
    angle inside [-pi, pi], the same flag outside the 1e-4 band of the threshold, the same state within the Acrobot bar."""
    assert search["count_mismatch"] == 0 and search["count_far"] == 0
    assert search["outside"] == 0
    assert search["done_mismatch"] == 0
    print({k: search[k] for k in ("dang", "lang", "dvel", "lvel")})
    assert search["dang"] <= 4 * search["lang"] and search["dvel"] <= 4 * search["lvel"]
    assert search["sum_dang"] <= 1.25 * search["sum_lang"]


def test_four_subtractions_fail_on_the_named_state(oracle):
    """The wrap this kernel had before: on "needs the fifth subtraction" four subtractions leave th1 outside [-pi, pi], a full turn
    away from where upstream's loop puts it; the k the twin and the kernel use now agrees with the loop."""
    s, a = T.ACROBOT_WORST["needs the fifth subtraction"]
    s = np.array(s, f32).reshape(4, 1)
    a = np.array([a], np.int32)
    four, now = oracle.acrobot_domain_probe(s, a, k=4), oracle.acrobot_domain_probe(s, a)
    assert four["wraps64"].max() == 5 and four["wrapsk"].max() == 4 and now["wrapsk"].max() == 5
    assert np.abs(four["nextk"][:2]).max() > T.PI32 and np.abs(now["nextk"][:2]).max() <= T.PI32
    assert np.abs(four["nextk"].astype(np.float64) - four["next64"])[:2].max() > 6.28
    assert np.abs(now["nextk"].astype(np.float64) - now["next64"])[:2].max() < 1e-3


def test_twin_wrap_cannot_hang_and_clamps_hand_nan_on(oracle):
    """Infinite and absurd angles end (the loop the twin had did not), and a NaN velocity stays NaN."""
    s = np.array([[np.inf, 0.1, 0.0, 0.0], [0.1, -np.inf, 0.0, 0.0], [1000.0, 0.1, 0.0, 0.0], [0.1, 0.1, np.nan, 0.0], [0.1, 0.1, 0.0, np.nan]], f32).T.copy()
    s2, obs, rw, d = oracle.acrobot_step(s, np.ones(5, np.int32), dtype=f32)
    assert not d.any()
    assert 960.0 < s2[0, 2] < 964.0                                              # 1000 - 6 * 2 pi = 962.3, and less than a radian of motion
    assert np.isnan(s2[2:, 3]).all() and np.isnan(s2[2:, 4]).all()
