"""CPU checks of the Box actor's policies (no GPU).  Fail without the feature: the library exports set_policy / get_policy and the header,
the ctypes mirror and Native.cs declare them with one arity; the recipe table of tests/_actor_box_policy_forms.py equals the
actor_box_policy_rollout_kernel forms in actor_box_policy.hip's gfx950 assembly, by name, both act kernels exist, and no kernel of the unit
spills or falls below two waves per SIMD; build.py lists the unit; Actor.SetPolicy / Actor.Policy refuse a Discrete actor and bad
arguments before any native call.  Pass without it (they test the yardstick): the statistics of the NumPy twin's normal draws — which
guard the choice of words: a u2 taken from word B would fail the exploring-lanes half — and the twin's bounds."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _actor_box_forms as box
import _actor_box_policy_forms as forms
import _actor_box_policy_twin as ptwin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CALLS = {"gymnet_vecenv_actor_box_set_policy": 4, "gymnet_vecenv_actor_box_get_policy": 4}


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


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,tick,lane0", [(7, 0, 0), (12345, 9, 1), (2 ** 40 + 3, 2 ** 33, 2 ** 32 + 5)])
def test_the_twins_normal_draws_have_mean_zero_and_variance_one(seed, tick, lane0):
    """5-sigma conditions on n standard normal draws: |mean| <= 5 / sqrt(n) (the mean's deviation is 1 / sqrt(n)) and |var - 1| <=
    5 * sqrt(2 / n) (the variance's is sqrt(2 / n)); over all lanes, and over the lanes that explore at epsilon = 0.1 — whose word B is
    small by construction, so a z that took its angle from word B would fail there."""
    n = 1 << 16
    a, b, noise = ptwin.words(seed, lane0, tick, n)
    z = ptwin.z64(a, noise)
    assert np.abs(z).max() <= 5.77
    assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1) <= 5 * np.sqrt(2 / n), (z.mean(), z.var())
    mask = ptwin.explore_mask(b, 0.1)
    m = int(mask.sum())
    assert 0.08 * n < m < 0.12 * n
    zs = z[mask]
    assert abs(zs.mean()) <= 5 / np.sqrt(m) and abs(zs.var() - 1) <= 5 * np.sqrt(2 / m), (m, zs.mean(), zs.var())
    biased = ptwin.z64(a, b)[mask]                                # the angle from the coin's own word: every cosine near 1
    assert abs(biased.mean()) > 5 / np.sqrt(m) or abs(biased.var() - 1) > 5 * np.sqrt(2 / m)


def test_the_words_are_picked_by_global_lane():
    """word (L & 3) of the call with counter (L >> 2, tick): a window that starts inside a group of four, past 2^32"""
    seed, tick, lane0 = 2 ** 40 + 3, 2 ** 33, 2 ** 32 + 5
    a, b, noise = ptwin.words(seed, lane0, tick, 9)
    from oracle import numpy_ref
    for i in range(9):
        lane = lane0 + i
        group = np.array([lane >> 2], np.uint64)
        assert noise[i] == numpy_ref.reset_words(seed ^ ptwin.NOISE_STREAM, group, tick)[lane & 3, 0]
        assert a[i] == numpy_ref.reset_words(seed ^ numpy_ref.ACTION_STREAM, group, tick)[lane & 3, 0]
        assert b[i] == numpy_ref.reset_words(seed ^ numpy_ref.AUX_STREAM, group, tick)[lane & 3, 0]
    assert ptwin.NOISE_STREAM not in (numpy_ref.ACTION_STREAM, numpy_ref.AUX_STREAM, 0)


@pytest.mark.parametrize("low,high", sorted(set(box.BOUNDS.values())))
def test_the_twins_heads_and_bounds(low, high):
    raw = np.array([-1e30, -3.0, -0.5, -0.0, 0.0, 0.25, 4.0, np.inf, np.nan], F32)
    g, gb = ptwin.greedy64(raw, low, high, "tanh")
    assert g[0] == low and g[7] == high and g[3] == 0 and g[4] == 0 and np.isnan(g[8])
    assert np.all((g[:8] >= low) & (g[:8] <= high)) and np.all(np.diff(g[:8]) >= 0)
    half = (high - low) / 2
    assert gb[0] == ptwin.tanh_bound(low, high) == half * 5 * 2.0 ** -24 + float(np.spacing(F32(high)))
    c, cb = ptwin.greedy64(raw, low, high, "clamp")
    assert np.array_equal(c[:8], np.clip(raw[:8].astype(np.float64), low, high)) and np.isnan(c[8]) and not cb.any()
    # sigma = 0: a Gaussian lane's value is its greedy value; the coin at epsilon = 1 takes every lane
    n = len(raw)
    wa, wb, wn = ptwin.words(3, 0, 0, n)
    act, bound, mask = ptwin.act64(raw, wa, wb, wn, 1.0, low, high, "tanh", "gaussian", 0.0)
    assert mask.all() and np.array_equal(act[:8], g[:8]) and np.isnan(act[8])
    # sigma > 0: inside the bounds, off the greedy value, and the bound grows by sigma * Z_BOUND and a spacing
    act, bound, mask = ptwin.act64(raw[:8], wa[:8], wb[:8], wn[:8], 1.0, low, high, "tanh", "gaussian", 0.5)
    assert np.all((act >= low) & (act <= high)) and (act != g[:8]).any()
    assert np.all(bound > gb[:8] + 0.5 * ptwin.Z_BOUND) and np.all(bound < gb[:8] + 0.5 * ptwin.Z_BOUND + 1e-6)
    # sample: the exploring lanes take tests/_actor_box_forms.py's draw, exactly
    act, bound, mask = ptwin.act64(raw[:8], wa[:8], wb[:8], wn[:8], 1.0, low, high, "tanh", "sample", 0.5)
    assert np.array_equal(act, box.sample(wa[:8], low, high).astype(np.float64)) and not bound.any()


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
    for c_name, py_name, value in (("GYMNET_BOX_HEAD_CLAMP", "BOX_HEAD_CLAMP", 0), ("GYMNET_BOX_HEAD_TANH", "BOX_HEAD_TANH", 1),
                                   ("GYMNET_BOX_EXPLORE_SAMPLE", "BOX_EXPLORE_SAMPLE", 0), ("GYMNET_BOX_EXPLORE_GAUSSIAN", "BOX_EXPLORE_GAUSSIAN", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (c_name, value), hdr) and getattr(capi, py_name) == value, c_name
    assert re.search(r"enum GymnetBoxHead \{ Clamp = 0, Tanh = 1 \}", native) and re.search(r"enum GymnetBoxExplore \{ Sample = 0, Gaussian = 1 \}", native)
    hpp = open(os.path.join(ROOT, "include", "gymnet_amd.hpp")).read()
    vcs = open(os.path.join(ROOT, "gym.net_amd", "csharp", "VectorEnv.cs")).read()
    for name in CALLS:
        assert name + "(" in hpp and "Native." + name + "(" in vcs, name
    for method in ("SetBoxActorPolicy", "GetBoxActorPolicy"):
        assert method + "(" in hpp and method + "(" in vcs, method
    # the header states the noise stream's constant, and it is philox.hpp's and the twin's
    assert "0x%016X" % ptwin.NOISE_STREAM in open(os.path.join(ROOT, "include", "gymnet_amd.h")).read()
    assert "kStreamNoise = 0x%016Xull" % ptwin.NOISE_STREAM in open(os.path.join(ROOT, "gym.net_amd", "csrc", "philox.hpp")).read()


@pytest.fixture(scope="module")
def unit_kernels():
    """{kernel name: resources} of actor_box_policy.hip compiled to gfx950 assembly with the product's flags (tools/kernel_resources.py)"""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "actor_box_policy.s")
        r = subprocess.run([kernel_resources.HIPCC] + kernel_resources.FLAGS + [os.path.join(kernel_resources.CSRC, "actor_box_policy.hip"), "-o", out],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return kernel_resources.kernels(out)


@pytest.mark.timeout(900)
def test_forms_table_names_every_compiled_policy_rollout_kernel(unit_kernels):
    compiled = sorted(n for n in unit_kernels if n.startswith("actor_box_policy_rollout_kernel<"))
    table = sorted(row["kernel"] for row in forms.FORMS)
    assert len(table) == len(set(table)) == 12
    assert compiled == table, (sorted(set(compiled) - set(table)), sorted(set(table) - set(compiled)))
    for row in forms.FORMS:                                       # each row says how to reach its kernel
        env, ar, extras, records = re.match(r"actor_box_policy_rollout_kernel<(\w+),(\w+),(\w+),(\w+)>", row["kernel"]).groups()
        assert forms.ENVS[env] == row["env"] and (ar == "true") == row["auto_reset"]
        assert (extras == "true", records == "true") == forms.SHAPES[row["shape"]]
    assert set(forms.ACT_KERNELS) <= set(unit_kernels)
    assert len(unit_kernels) == 14                                # the unit compiles nothing else
    assert all(p[:2] != ("clamp", "sample") for p in forms.POLICIES)   # ... and the default policy does not reach it


@pytest.mark.timeout(900)
def test_policy_kernels_do_not_spill_and_keep_two_waves(unit_kernels):
    assert unit_kernels
    for n in sorted(unit_kernels):
        assert unit_kernels[n]["scratch"] == 0, (n, unit_kernels[n])
        assert unit_kernels[n]["occupancy"] >= 2, (n, unit_kernels[n])


def test_the_unit_is_a_build_input():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    assert "actor_box_policy.hip" in kernel_resources._BUILD.SOURCES and "actor_box_policy.hip" in kernel_resources._BUILD.DEPS
    assert "actor_net.hpp" in kernel_resources._BUILD.DEPS and "philox.hpp" in kernel_resources._BUILD.DEPS


def test_set_policy_and_policy_check_their_arguments_before_any_native_call(gymnet):
    import importlib
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")

    class NoNativeCalls:
        def __getattr__(self, name):
            raise AssertionError("native call: " + name)

    def bare(is_box):
        o = ve.Actor.__new__(ve.Actor)
        o.__dict__.update(IsBox=is_box, _lib=NoNativeCalls(), _h=1, _env=type("Env", (), {"_h": 1})())
        return o
    discrete = bare(False)
    with pytest.raises(ValueError):
        discrete.SetPolicy("tanh", "gaussian", 0.3)
    with pytest.raises(ValueError):
        discrete.SetPolicy()
    with pytest.raises(ValueError):
        discrete.Policy
    actor = bare(True)
    for args in (("softmax", "sample", 0.0), ("tanh", "normal", 0.0), (1, "sample", 0.0), ("tanh", None, 0.0), ("tanh", "gaussian", float("nan")),
                 ("tanh", "gaussian", -1.0), ("tanh", "gaussian", float("inf")), ("clamp", "sample", -0.5)):
        with pytest.raises(ValueError):
            actor.SetPolicy(*args)
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_box_set_policy"):     # good arguments do reach the library
        actor.SetPolicy("tanh", "gaussian", 0.3)
