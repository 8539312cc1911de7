"""CPU checks of a Discrete actor's softmax exploration (no GPU).  Fail without the feature: the library exports set_exploration /
get_exploration and the header, the ctypes mirror and Native.cs declare them with one arity; the recipe table of
tests/_actor_softmax_forms.py equals the actor_softmax_rollout_kernel forms in actor_softmax.hip's gfx950 assembly, by name, the three act
kernels exist, and every kernel of the unit stays within a few VGPRs of its actor.hip sibling, at its occupancy and LDS, with no scratch
where the sibling has none; build.py lists the unit; Actor.SetExploration / Actor.Exploration refuse a Box actor and bad arguments before
any native call.  Pass without it (they test the yardstick): the C twin (tests/_actor_softmax_twin.py) against float64 — exp_neg over
every float32 in [-104, 0] and the normalised cumulative distribution over two million random cases within 2^-20 —, the statistics of
its draws — which guard the choice of word: a u taken from word B misses the exploring-lanes half — and hand-worked edges."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _actor_softmax_forms as forms
import _actor_softmax_twin as stwin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CALLS = {"gymnet_vecenv_actor_set_exploration": 3, "gymnet_vecenv_actor_get_exploration": 3}
U_MAX = F32(16777215.0 / 16777216.0)                              # the largest value of u01_24


def _split_args(argtext):
    out, depth, cur = [], 0, ""
    for ch in argtext:
        depth += ch in "([{<"
        depth -= ch in ")]}>"
        if ch == "," and depth == 0:
            out.append(cur.strip()); cur = ""
        else:
            cur += ch
    return out + ([cur.strip()] if cur.strip() else [])


# ---- the yardstick: the twin against float64 -------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_exp_neg_over_every_float32_in_minus_104_to_0():
    """Worst absolute error against the double exp, measured: 5.5e-8 (at arguments near 0, where exp is near 1 and half an ulp of the
    result is 3e-8).  The bound: 2^-23, one ulp of a result in [0.5, 1) — a degree-7 Taylor remainder of 5e-9 relative, the product by
    log2 e rounded once (|t| * 2^-24 * ln 2 relative, 3e-8 absolute at its worst near t = -1.44) and a Horner chain of seven fmaf."""
    hi = int(np.array([104.0], F32).view(np.uint32)[0])
    edges = np.linspace(0, hi + 1, 17).astype(np.int64)
    with ThreadPoolExecutor(16) as ex:                               # (ctypes releases the GIL)
        res = list(ex.map(lambda k: stwin.exp_neg_sweep(int(edges[k]), int(edges[k + 1] - 1)), range(16)))
    worst = max(r[0] for r in res)
    print(f"exp_neg over {hi + 1} arguments: worst absolute error {worst:.3e}")
    assert worst <= 2.0 ** -23
    # the cut: the scaled argument must be >= -125; below it (and for a NaN) the value is exactly +0
    edge = np.array([0.0, -0.0, -86.6, -86.7, -104.0, -1e30, -np.inf, np.nan], F32)
    got = stwin.exp_neg(edge)
    assert got[0] == 1.0 and got[1] == 1.0 and got[2] > 0 and np.array_equal(got[3:].view(np.uint32), np.zeros(5, np.uint32))
    assert got[2] >= np.finfo(F32).tiny                             # normal down to the cut


def test_the_twins_cumulative_distribution_is_within_2_to_the_minus_20_of_float64():
    """Two million random cases: A in 2..8, logits uniform in +-10, temperature in {0.1, 1, 5}; c_k / S against the cumulative float64
    softmax of the same float32 logits.  Measured worst: 2.7e-7 (under a third of the bound)."""
    rng = np.random.default_rng(20)
    worst, cases = 0.0, 0
    for A in range(2, 9):
        for tau in (0.1, 1.0, 5.0):
            n = 2_000_000 // 21 + 1
            logits = rng.uniform(-10, 10, (n, A)).astype(F32)
            action, greedy, c = stwin.draw(logits, rng.random(n).astype(F32), tau)
            want = np.cumsum(stwin.softmax64(logits, tau), axis=1)
            err = np.abs(c.astype(np.float64) / c[:, -1:].astype(np.float64) - want).max()
            worst, cases = max(worst, err), cases + n
            assert np.array_equal(greedy, np.argmax(logits, axis=1))
            assert ((action >= 0) & (action < A)).all()
    print(f"{cases} cases: worst CDF error {worst:.3e} (bound {stwin.CDF_BOUND:.3e})")
    assert cases >= 2_000_000 and worst <= stwin.CDF_BOUND


LOGITS = np.array([0.3, -1.2, 1.1, 0.0, -0.4], F32)               # one fixed logit vector, five actions


def _five_sigma(actions, p):
    """every action's count within 5 binomial standard deviations of n * p"""
    n = len(actions)
    counts = np.bincount(actions, minlength=len(p)).astype(np.float64)
    return bool(np.all(np.abs(counts - n * p) <= 5.0 * np.sqrt(n * p * (1.0 - p))))


@pytest.mark.parametrize("temperature", [1.0, 0.5])
@pytest.mark.parametrize("seed,tick,lane0", [(7, 0, 0), (12345, 9, 1), (2 ** 40 + 3, 2 ** 33, 2 ** 32 + 5)])
def test_the_twins_draws_follow_the_float64_probabilities(seed, tick, lane0, temperature):
    """2^16 lanes, one logit vector: the action frequencies meet the 5-sigma binomial condition against the float64 softmax over all lanes
    at epsilon = 1 and over the exploring lanes at epsilon = 0.1 — whose word B is small by construction, so the same draw with u taken
    from word B piles onto action 0 and misses."""
    n = 1 << 16
    logits = np.tile(LOGITS, (n, 1))
    p = stwin.softmax64(LOGITS[None], temperature)[0]
    a, b = stwin.words(seed, lane0, tick, n)
    act, mask, greedy = stwin.act(logits, a, b, 1.0, "softmax", temperature)
    assert mask.all() and (greedy == 2).all()
    assert _five_sigma(act, p), (np.bincount(act, minlength=5) / n, p)
    act, mask, _ = stwin.act(logits, a, b, 0.1, "softmax", temperature)
    m = int(mask.sum())
    assert 0.08 * n < m < 0.12 * n
    assert (act[~mask] == 2).all()                                  # a lane that does not explore takes the argmax
    assert _five_sigma(act[mask], p), (np.bincount(act[mask], minlength=5) / m, p)
    biased, _, _ = stwin.act(logits, a, b, 0.1, "softmax", temperature, u_words=b)
    assert not _five_sigma(biased[mask], p)
    assert (biased[mask] == 0).mean() > 0.5


def test_hand_worked_edges():
    u = np.array([0.0, 0.25, 0.5, 0.75, U_MAX], F32)
    # equal logits, A = 2 and A = 8: e_k = 1, c_k = k + 1, the action is floor(u * A); the greedy action is the first index
    for A in (2, 8):
        act, greedy, c = stwin.draw(np.zeros((5, A), F32), u, 1.0)
        assert (greedy == 0).all() and np.array_equal(c[0], np.arange(1, A + 1, dtype=F32))
        assert np.array_equal(act, np.floor(u.astype(np.float64) * A).astype(np.int32)) and act[-1] == A - 1
    # a gap above 104 * tau: the far action's weight is exactly +0 and it is never chosen, also by the lane whose u is the largest
    for tau in (0.25, 1.0, 4.0):
        gap = F32(104.5 * tau)
        logits = np.tile(np.array([0.0, -gap, 0.0], F32), (5, 1))
        act, greedy, c = stwin.draw(logits, u, tau)
        assert np.array_equal(c[0], np.array([1.0, 1.0, 2.0], F32)) and not (act == 1).any()
        assert np.array_equal(act, np.array([0, 0, 2, 2, 2], np.int32))
        logits = np.tile(np.array([0.0, 0.0, -gap], F32), (5, 1))            # ... as the last action: thr < c_1 = S always holds
        act, _, c = stwin.draw(logits, u, tau)
        assert c[0, 2] == c[0, 1] == 2.0 and not (act == 2).any() and act[-1] == 1
    # the largest u: u_max * S stays below S (S * 2^-24 is more than half a spacing of S unless S is a power of two, where the product is
    # exact), so the lane takes the last action with a positive weight, not an index past the end
    act, greedy, c = stwin.draw(np.array([[-1.0, 0.5, 0.25]], F32), np.array([U_MAX], F32), 1.0)
    assert U_MAX * c[0, 2] < c[0, 2] and act[0] == 2 and greedy[0] == 1
    # S = 0: +-inf and NaN logits give the greedy action whatever u is
    for row, g in (([np.inf, 0.0, np.inf], 0), ([-np.inf, -np.inf, -np.inf], 0), ([np.nan, 1.0, 2.0], 0), ([0.0, np.inf], 1)):
        logits = np.tile(np.array(row, F32), (5, 1))
        act, greedy, c = stwin.draw(logits, u, 1.0)
        assert (greedy == g).all() and (c[:, -1] == 0).all() and np.array_equal(act, greedy), row
    # a NaN beside finite logits has weight 0 and is never chosen
    logits = np.tile(np.array([1.0, np.nan, 1.0], F32), (5, 1))
    act, greedy, c = stwin.draw(logits, u, 1.0)
    assert np.array_equal(c[0], np.array([1.0, 1.0, 2.0], F32)) and np.array_equal(act, np.array([0, 0, 2, 2, 2], np.int32))
    # the uniform rule and the coin
    assert np.array_equal(stwin.uniform(np.array([0, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], np.uint32), 3), np.array([0, 1, 1, 2], np.int32))
    assert stwin.coin_threshold(0.0) == 0xFF and stwin.coin_threshold(1.0) == 0xFFFFFFFF
    assert stwin.inv_tau(0.5) == 2.0 and stwin.inv_tau(0.1) == F32(1.0) / F32(0.1)


def test_a_low_temperature_sharpens_and_a_high_one_flattens():
    n = 1 << 14
    rng = np.random.default_rng(3)
    u = rng.random(n).astype(F32)
    logits = np.tile(LOGITS, (n, 1))
    share = [float((stwin.draw(logits, u, tau)[0] == 2).mean()) for tau in (0.1, 1.0, 5.0)]
    assert share[0] > 0.99 and share[0] > share[1] > share[2] > 0.2


# ---- fail without the feature -----------------------------------------------------------------------------------------------------
def test_both_calls_are_exported_and_declared_with_one_arity(gymnet):
    import importlib
    capi = importlib.import_module(gymnet.__name__ + "._capi")
    lib = ctypes.CDLL(gymnet.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gymnet_amd.h")).read(), flags=re.S)
    native = re.sub(r"//.*", "", open(os.path.join(ROOT, "gym.net_amd", "csharp", "Native.cs")).read())
    for name, arity in CALLS.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        assert name in capi.PROTOTYPES
        assert len(capi.PROTOTYPES[name][1]) == len(_split_args(m.group(1))) == arity, name
        cs = re.search(r"\[DllImport\(Lib\)\] public static extern int %s\(([^;]*)\);" % name, native)
        assert cs and len(_split_args(cs.group(1))) == arity, name
    assert capi.ABI_VERSION == 6
    assert re.search(r"#define\s+GYMNET_ABI_VERSION\s+6\b", hdr)
    for c_name, py_name, value in (("GYMNET_ACTOR_EXPLORE_UNIFORM", "ACTOR_EXPLORE_UNIFORM", 0), ("GYMNET_ACTOR_EXPLORE_SOFTMAX", "ACTOR_EXPLORE_SOFTMAX", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (c_name, value), hdr) and getattr(capi, py_name) == value, c_name
    assert re.search(r"enum GymnetActorExplore \{ Uniform = 0, Softmax = 1 \}", native)
    hpp = open(os.path.join(ROOT, "include", "gymnet_amd.hpp")).read()
    vcs = open(os.path.join(ROOT, "gym.net_amd", "csharp", "VectorEnv.cs")).read()
    for name in CALLS:
        assert name + "(" in hpp and "Native." + name + "(" in vcs, name
    for method in ("SetActorExploration", "GetActorExploration"):
        assert method + "(" in hpp and method + "(" in vcs, method


def test_exp_neg_header_and_twin_share_their_constants():
    """the C twin restates csrc/exp_neg.hpp: the same literals, the same cut, the same chain length"""
    hpp = open(os.path.join(ROOT, "gym.net_amd", "csrc", "exp_neg.hpp")).read()
    lits = re.findall(r"=\s*([0-9.]+f)\b", hpp)
    assert len(lits) == 8
    for lit in lits:
        assert lit in stwin.C_SRC, lit
    assert hpp.count("__builtin_fmaf(") == stwin.C_SRC.count("fmaf(p, f") == 7
    assert "t >= -125.0f" in hpp and "t >= -125.0f" in stwin.C_SRC and "__builtin_rintf(t)" in hpp and "rintf(t)" in stwin.C_SRC


@pytest.fixture(scope="module")
def unit_kernels():
    """({kernel name: resources} of actor_softmax.hip, the same of actor.hip), both compiled to gfx950 assembly with the product's flags
    (tools/kernel_resources.py)"""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    with tempfile.TemporaryDirectory() as d:
        def compile_unit(unit):
            out = os.path.join(d, unit + ".s")
            r = subprocess.run([kernel_resources.HIPCC] + kernel_resources.FLAGS + [os.path.join(kernel_resources.CSRC, unit + ".hip"), "-o", out],
                               capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            return kernel_resources.kernels(out)
        with ThreadPoolExecutor(2) as ex:
            return tuple(ex.map(compile_unit, ("actor_softmax", "actor")))


@pytest.mark.timeout(900)
def test_forms_table_names_every_compiled_softmax_rollout_kernel(unit_kernels):
    kernels, _ = unit_kernels
    compiled = sorted(n for n in kernels if n.startswith("actor_softmax_rollout_kernel<"))
    table = sorted(row["kernel"] for row in forms.FORMS)
    assert len(table) == len(set(table)) == 18
    assert compiled == table, (sorted(set(compiled) - set(table)), sorted(set(table) - set(compiled)))
    for row in forms.FORMS:                                       # each row says how to reach its kernel
        env, ar, extras, records = re.match(r"actor_softmax_rollout_kernel<(\w+),(\w+),(\w+),(\w+)>", row["kernel"]).groups()
        assert forms.ENVS[env] == row["env"] and (ar == "true") == row["auto_reset"]
        assert (extras == "true", records == "true") == forms.SHAPES[row["shape"]]
    assert set(forms.ACT_KERNELS) <= set(kernels)
    assert len(kernels) == 21                                     # the unit compiles nothing else
    assert forms.SETTINGS[0] == ("uniform", 1.0) and all(s[0] == "softmax" for s in forms.SETTINGS[1:])


@pytest.mark.timeout(900)
def test_softmax_kernels_stay_within_their_siblings_budget(unit_kernels):
    """a few VGPRs (4, the margin the Box policy unit was held to) above the actor.hip sibling at the most, the sibling's waves per SIMD and
    LDS, and no scratch where the sibling has none"""
    kernels, siblings = unit_kernels
    assert len(kernels) == 21
    for n in sorted(kernels):
        k, s = kernels[n], siblings[forms.SIBLING[n]]
        print(f"{n:64s} VGPRs {k['vgpr']:3d} (sibling {s['vgpr']:3d})  scratch {k['scratch']} ({s['scratch']})  LDS {k['lds']} ({s['lds']})")
        assert k["vgpr"] <= s["vgpr"] + 4, (n, k, s)
        assert k["occupancy"] >= s["occupancy"] and k["occupancy"] >= 2, (n, k, s)
        assert k["lds"] == s["lds"], (n, k, s)
        assert k["scratch"] <= s["scratch"], (n, k, s)             # 0 wherever the sibling's is 0


def test_the_profile_lists_the_compiled_kernels():
    text = open(os.path.join(ROOT, "profiles", "kernel_resources_actor_softmax.txt")).read()
    for name in [row["kernel"] for row in forms.FORMS] + list(forms.ACT_KERNELS):
        assert re.search(r"^%s\s+\d+\s+\d+\s+\d+\s+\d+$" % re.escape(name), text, flags=re.M), name


def test_the_unit_is_a_build_input():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    assert "actor_softmax.hip" in kernel_resources._BUILD.SOURCES and "actor_softmax.hip" in kernel_resources._BUILD.DEPS
    assert "exp_neg.hpp" in kernel_resources._BUILD.DEPS and "actor_net.hpp" in kernel_resources._BUILD.DEPS


def test_set_exploration_checks_its_arguments_before_any_native_call(gymnet):
    import importlib
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")

    class NoNativeCalls:
        def __getattr__(self, name):
            raise AssertionError("native call: " + name)

    def bare(is_box):
        o = ve.Actor.__new__(ve.Actor)
        o.__dict__.update(IsBox=is_box, _lib=NoNativeCalls(), _h=1, _env=type("Env", (), {"_h": 1})())
        return o
    box = bare(True)
    with pytest.raises(ValueError, match="Box"):
        box.SetExploration("softmax", 1.0)
    with pytest.raises(ValueError, match="Box"):
        box.SetExploration()
    with pytest.raises(ValueError, match="Box"):
        box.Exploration
    actor = bare(False)
    for args in (("gaussian", 1.0), ("Softmax", 1.0), (1, 1.0), (True, 1.0), (None, 1.0), ("softmax", True), ("softmax", float("nan")),
                 ("softmax", 0.0), ("softmax", -1.0), ("softmax", float("inf")), ("softmax", 1e-39), ("softmax", 1e-50), ("uniform", 0.0),
                 ("softmax", 1e39)):
        with pytest.raises(ValueError):
            actor.SetExploration(*args)
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_set_exploration"):     # good arguments do reach the library
        actor.SetExploration("softmax", 0.5)
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_set_exploration"):
        actor.SetExploration("softmax", 3e-39)                                                         # 1 / it is finite in float32
