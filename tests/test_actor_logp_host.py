"""CPU checks of the log-probability a Discrete actor records (no GPU).  Fail without the feature: the library exports
gymnet_vecenv_actor_act_logp_device / gymnet_vecenv_rollout_fused_logp_device and the header, the ctypes mirror, Native.cs, the .hpp and
VectorEnv.cs declare them with one arity, at ABI 6; the recipe table of tests/_actor_logp_forms.py equals the actor_logp_rollout_kernel
forms in actor_logp.hip's gfx950 assembly, by name, the three act kernels exist, the unit compiles 21 kernels, and every one of them keeps
its actor_softmax.hip sibling's waves per SIMD and LDS with no scratch where the sibling has none; csrc/log_pos.hpp and the twin share
their literals; build.py lists the unit and its headers; Act(logp=) and RolloutFusedDevice(rec_logp=) refuse a Box actor, a wrong dtype /
shape / device and a non-actor action source before any native call; the profile lists every compiled kernel.  Pass without it (they test
the yardstick): log_pos over every float32 in [1, 8] — exactly +0 at 1, never below +0, non-decreasing, within 2^-21 of the float64 log —,
the twin's logp against the float64 log-softmax over two million random cases within 2^-20 * max(1, |logp|), and hand-worked edges."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _actor_logp_forms as forms
import _actor_logp_twin as ltwin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CALLS = {"gymnet_vecenv_actor_act_logp_device": 7, "gymnet_vecenv_rollout_fused_logp_device": 3}
NAN = np.uint32(ltwin.NAN_BITS)
NEG_INF = np.array([-np.inf], F32).view(np.uint32)[0]


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


def _bits(x):
    return np.asarray(x, F32).view(np.uint32)


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_log_pos_over_every_float32_in_1_to_8():
    """3 * 2^23 + 1 arguments, in 16 runs side by side, each handed the result of the argument before its first one so that the order is
    checked across the seams.  Measured worst absolute error against the double log: 1.20e-7 (half a spacing of float32 at ln 8 = 2.08,
    where the results are coarsest); the bound 2^-21 is two spacings there."""
    lo, hi = int(_bits([1.0])[0]), int(_bits([8.0])[0])
    assert hi - lo + 1 == 3 * 2 ** 23 + 1
    edges = np.linspace(lo, hi + 1, 17).astype(np.int64)
    prev = [None] + [float(ltwin.log_pos(np.array([edges[k] - 1], np.uint32).view(F32))[0]) for k in range(1, 16)]
    with ThreadPoolExecutor(16) as ex:                               # (ctypes releases the GIL)
        res = list(ex.map(lambda k: ltwin.log_pos_sweep(int(edges[k]), int(edges[k + 1] - 1), prev[k]), range(16)))
    worst, decreasing, below = max(r[0] for r in res), sum(r[1] for r in res), sum(r[2] for r in res)
    print(f"log_pos over {hi - lo + 1} arguments: worst absolute error {worst:.3e} (bound {ltwin.LOG_POS_BOUND:.3e}), "
          f"{decreasing} decreasing, {below} below +0")
    assert _bits(ltwin.log_pos([1.0]))[0] == 0                       # exactly +0.0f
    assert below == 0
    assert decreasing == 0
    assert worst <= ltwin.LOG_POS_BOUND
    assert res[-1][3] == ltwin.log_pos([8.0])[0] and abs(float(res[-1][3]) - np.log(8.0)) <= ltwin.LOG_POS_BOUND


def test_the_twins_logp_is_within_2_to_the_minus_20_of_the_float64_log_softmax():
    """Over two million random cases: A in 2..8, logits uniform in +-10, temperature in {0.1, 1, 5}, every action of every case; the
    condition is |error| <= 2^-20 * max(1, |logp64|) against the float64 log-softmax of the same float32 logits at the true temperature.
    Measured worst of error / max(1, |logp64|): 3.0e-7 (bound 9.54e-7), which is what a correctly rounded logarithm in log_pos's place
    gives too: the error is the product's and the subtraction's, at |logp| near 100."""
    rng = np.random.default_rng(21)
    worst, cases = 0.0, 0
    for A in range(2, 9):
        for tau in (0.1, 1.0, 5.0):
            n = 2_000_000 // 21 + 1
            logits = rng.uniform(-10, 10, (n, A)).astype(F32)
            want = ltwin.log_softmax64(logits, tau)
            for j in range(A):
                got = ltwin.logp(logits, np.full(n, j, np.int32), tau).view(F32).astype(np.float64)
                assert np.isfinite(got).all() and (got <= 0).all()
                worst = max(worst, float((np.abs(got - want[:, j]) / np.maximum(1.0, np.abs(want[:, j]))).max()))
            cases += n
    print(f"{cases} cases, every action: worst |error| / max(1, |logp64|) {worst:.3e} (bound {ltwin.LOGP_BOUND:.3e})")
    assert cases >= 2_000_000 and worst <= ltwin.LOGP_BOUND


def test_hand_worked_edges():
    # equal logits, A = 2 and A = 8: every action's logp has the bits of -log_pos(A), within the bound of -ln A
    for A in (2, 8):
        logits = np.full((A, A), 0.75, F32)
        got = ltwin.logp(logits, np.arange(A, dtype=np.int32), 1.0)
        want = -ltwin.log_pos([float(A)])[0]
        assert (got == _bits([want])[0]).all(), (A, got)
        assert abs(float(want) + np.log(A)) <= ltwin.LOGP_BOUND * max(1.0, np.log(A))
    # a gap above 104 * tau: the greedy action's logp is +0.0f (S = 1, log_pos(1) = +0, 0 - 0), the far action's is a_far - 0, finite
    for tau in (0.25, 1.0, 4.0):
        gap = F32(104.5 * tau)
        logits = np.tile(np.array([0.0, -gap], F32), (2, 1))
        got = ltwin.logp(logits, np.array([0, 1], np.int32), tau)
        a_far = (F32(-gap) - F32(0.0)) * ltwin.inv_tau(tau)
        assert got[0] == 0 and got[1] == _bits([a_far])[0] and np.isfinite(a_far) and a_far < -104.0
    # +inf or a NaN as the greedy logit: the canonical NaN for every action
    for row in ([np.inf, 0.0, 1.0], [0.0, np.inf, np.inf], [np.nan, 1.0, 2.0], [-np.inf, -np.inf, -np.inf]):
        logits = np.tile(np.array(row, F32), (3, 1))
        assert (ltwin.logp(logits, np.arange(3, dtype=np.int32), 1.0) == NAN).all(), row
    # a -inf logit beside finite ones: -inf for that action, finite for the others
    logits = np.tile(np.array([0.5, -np.inf, 0.25], F32), (3, 1))
    got = ltwin.logp(logits, np.arange(3, dtype=np.int32), 1.0)
    assert got[1] == NEG_INF and np.isfinite(got[[0, 2]].view(F32)).all()
    # a NaN logit beside finite ones (never the greedy one: the argmax moves on a strictly greater value only, and starts at index 0)
    logits = np.tile(np.array([0.5, np.nan, 0.25], F32), (3, 1))
    got = ltwin.logp(logits, np.arange(3, dtype=np.int32), 1.0)
    assert got[1] == NAN and np.isfinite(got[[0, 2]].view(F32)).all()
    # no result is above +0: random rows, every action, three temperatures, and rows with small gaps
    rng = np.random.default_rng(5)
    for A in (2, 3, 8):
        for scale in (1e-6, 1e-3, 1.0, 30.0):
            logits = (rng.standard_normal((4096, A)) * scale).astype(F32)
            for tau in (0.1, 1.0, 5.0):
                for j in range(A):
                    got = ltwin.logp(logits, np.full(4096, j, np.int32), tau).view(F32)
                    assert (got <= 0).all()


# ---- fail without the feature -----------------------------------------------------------------------------------------------------
def test_both_calls_are_exported_and_declared_with_one_arity(gymnet):
    import importlib
    capi = importlib.import_module(gymnet.__name__ + "._capi")
    lib = ctypes.CDLL(gymnet.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gymnet_amd.h")).read(), flags=re.S)
    native = re.sub(r"//.*", "", open(os.path.join(ROOT, "gym.net_amd", "csharp", "Native.cs")).read())
    hpp = open(os.path.join(ROOT, "include", "gymnet_amd.hpp")).read()
    vcs = open(os.path.join(ROOT, "gym.net_amd", "csharp", "VectorEnv.cs")).read()
    for name, arity in CALLS.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        assert name in capi.PROTOTYPES
        assert len(capi.PROTOTYPES[name][1]) == len(_split_args(m.group(1))) == arity, name
        cs = re.search(r"\[DllImport\(Lib\)\] public static extern int %s\(([^;]*)\);" % name, native)
        assert cs and len(_split_args(cs.group(1))) == arity, name
        call = re.search(name + r"\(([^;]*)\)\);", hpp)
        assert call and len(_split_args(call.group(1))) == arity, name
        call = re.search(r"Native\." + name + r"\(([^;]*)\)\);", vcs)
        assert call and len(_split_args(call.group(1))) == arity, name
    assert capi.ABI_VERSION == 6
    assert re.search(r"#define\s+GYMNET_ABI_VERSION\s+6\b", hdr)
    for method in ("ActorActLogp", "RolloutFusedLogp"):
        assert method + "(" in hpp and method + "(" in vcs, method


def test_log_pos_header_and_twin_share_their_constants():
    """the C twin restates csrc/log_pos.hpp: the same literals, the same integer constants, the same chain length"""
    hpp = open(os.path.join(ROOT, "gym.net_amd", "csrc", "log_pos.hpp")).read()
    code = hpp[hpp.index("#pragma once"):]
    lits = re.findall(r"=\s*(-?[0-9.]+(?:e-?[0-9]+)?f)\b", code)
    assert len(lits) == 11                                          # ln2_hi, ln2_lo and the nine coefficients
    for lit in lits:
        assert lit in ltwin.C_SRC, lit
    for word in ("0x3f3504f3", "0x3f800000", "0x007fffff", ">> 23) - 127"):
        assert word in code and word in ltwin.C_SRC, word
    assert code.count("__builtin_fmaf(p, f,") == ltwin.C_SRC.count("fmaf(p, f, p") == 8
    assert code.count("__builtin_fmaf(") == 10 and "logf" not in code and "__builtin_amdgcn" not in code
    exp_neg = open(os.path.join(ROOT, "gym.net_amd", "csrc", "exp_neg.hpp")).read()
    for lit in re.findall(r"=\s*([0-9.]+f)\b", exp_neg):            # ... and the twin's exp_neg is exp_neg.hpp's
        assert lit in ltwin.C_SRC, lit


@pytest.fixture(scope="module")
def unit_kernels():
    """({kernel name: resources} of actor_logp.hip, the same of actor_softmax.hip), both compiled to gfx950 assembly with the product's
    flags (tools/kernel_resources.py)"""
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
            return tuple(ex.map(compile_unit, ("actor_logp", "actor_softmax")))


@pytest.mark.timeout(900)
def test_forms_table_names_every_compiled_logp_rollout_kernel(unit_kernels):
    kernels, _ = unit_kernels
    compiled = sorted(n for n in kernels if n.startswith("actor_logp_rollout_kernel<"))
    table = sorted(row["kernel"] for row in forms.FORMS)
    assert len(table) == len(set(table)) == 18
    assert compiled == table, (sorted(set(compiled) - set(table)), sorted(set(table) - set(compiled)))
    for row in forms.FORMS:                                       # each row says how to reach its kernel
        env, ar, extras, records = re.match(r"actor_logp_rollout_kernel<(\w+),(\w+),(\w+),(\w+)>", row["kernel"]).groups()
        assert forms.ENVS[env] == row["env"] and (ar == "true") == row["auto_reset"]
        assert (extras == "true", records == "true") == forms.SHAPES[row["shape"]]
    assert set(forms.ACT_KERNELS) <= set(kernels)
    assert len(kernels) == 21                                     # the unit compiles nothing else


@pytest.mark.timeout(900)
def test_logp_kernels_keep_their_siblings_occupancy_and_lds_without_scratch(unit_kernels):
    """against the actor_softmax.hip sibling: waves per SIMD not below it and >= 2, equal LDS, no scratch where it has none.  The VGPR
    counts are listed (and kept in profiles/kernel_resources_actor_logp.txt), not asserted beyond what the occupancy implies."""
    kernels, siblings = unit_kernels
    assert len(kernels) == 21
    for n in sorted(kernels):
        k, s = kernels[n], siblings[forms.SIBLING[n]]
        print(f"{n:64s} VGPRs {k['vgpr']:3d} (sibling {s['vgpr']:3d})  waves {k['occupancy']} ({s['occupancy']})  scratch {k['scratch']} ({s['scratch']})  "
              f"LDS {k['lds']} ({s['lds']})")
        assert k["occupancy"] >= s["occupancy"] and k["occupancy"] >= 2, (n, k, s)
        assert k["lds"] == s["lds"], (n, k, s)
        assert k["scratch"] <= s["scratch"], (n, k, s)             # 0 wherever the sibling's is 0


def test_the_profile_lists_the_compiled_kernels():
    text = open(os.path.join(ROOT, "profiles", "kernel_resources_actor_logp.txt")).read()
    for name in [row["kernel"] for row in forms.FORMS] + list(forms.ACT_KERNELS):
        assert re.search(r"^%s\s+\d+\s+\d+\s+\d+\s+\d+$" % re.escape(name), text, flags=re.M), name


def test_the_unit_is_a_build_input():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    assert "actor_logp.hip" in kernel_resources._BUILD.SOURCES and "actor_logp.hip" in kernel_resources._BUILD.DEPS
    for header in ("log_pos.hpp", "exp_neg.hpp", "actor_net.hpp"):
        assert header in kernel_resources._BUILD.DEPS, header


class _Tensor:
    """what the argument checks look at, without a GPU"""

    def __init__(self, shape, dtype="torch.float32", cuda=True, contiguous=True):
        self.shape, self.dtype, self.is_cuda, self._contiguous = tuple(shape), dtype, cuda, contiguous

    def data_ptr(self):
        return 4096

    def is_contiguous(self):
        return self._contiguous


class NoNativeCalls:
    def __getattr__(self, name):
        raise AssertionError("native call: " + name)


def test_logp_arguments_are_checked_before_any_native_call(gymnet):
    import importlib
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")
    N, T = 12, 5

    def bare_env(actor_is_box=None):
        env = ve.VectorEnv.__new__(ve.VectorEnv)
        env.__dict__.update(_lib=NoNativeCalls(), _h=1, _owns_handle=False, NumberOfEnvironments=N, Device=0)
        if actor_is_box is not None:
            env._actor = bare_actor(actor_is_box, env)
        return env

    def bare_actor(is_box, env=None):
        o = ve.Actor.__new__(ve.Actor)
        o.__dict__.update(IsBox=is_box, _lib=NoNativeCalls(), _h=1, _env=env or bare_env(), _out=_Tensor((N,), "torch.int32"))
        return o

    out = _Tensor((N,), "torch.int32")
    with pytest.raises(ValueError, match="Box"):
        bare_actor(True).Act(0.0, out=out, logp=_Tensor((N,)))
    with pytest.raises(ValueError, match="Box"):
        bare_actor(True).Step(0.0, logp=_Tensor((N,)))
    actor = bare_actor(False)
    bad = (_Tensor((N,), "torch.float64"), _Tensor((N,), "torch.int32"), _Tensor((N + 1,)), _Tensor((N, 1)), _Tensor((1, N)), _Tensor(()),
           _Tensor((N,), cuda=False), _Tensor((N,), contiguous=False), np.zeros(N, F32), 4096, [0.0] * N)
    for logp in bad:
        with pytest.raises(ValueError):
            actor.Act(0.0, out=out, logp=logp)
        with pytest.raises(ValueError):
            actor.Step(0.0, logp=logp)
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_act_logp_device"):      # good arguments do reach the library
        actor.Act(0.0, out=out, logp=_Tensor((N,)))
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_act_logp_device"):
        actor.Step(0.0, repeat=2, logp=_Tensor((N,)))
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_act_device"):           # ... and without logp the old call
        actor.Act(0.0, out=out)
    good = _Tensor((T, N))
    with pytest.raises(ValueError, match="Box"):
        bare_env(True).RolloutFusedDevice(None, T, actions="actor", rec_logp=good)
    with pytest.raises(ValueError, match="actor"):
        bare_env().RolloutFusedDevice(None, T, actions="actor", rec_logp=good)                          # no actor at all
    env = bare_env(False)
    for source in ("ring", "sample", "epsilon_greedy"):
        with pytest.raises(ValueError, match="actor"):
            env.RolloutFusedDevice(_Tensor((T, N), "torch.int32"), T, actions=source, rec_logp=good)
    for rec in (_Tensor((T, N), "torch.float64"), _Tensor((T, N), "torch.float16"), _Tensor((T + 1, N)), _Tensor((T, N + 1)), _Tensor((N, T)),
                _Tensor((T * N,)), _Tensor((T, N), cuda=False), _Tensor((T, N), contiguous=False), np.zeros((T, N), F32), 4096):
        with pytest.raises(ValueError):
            env.RolloutFusedDevice(None, T, actions="actor", rec_logp=rec)
    with pytest.raises(ValueError):
        env.RolloutFusedDevice(None, T, actions="actor", rec_logp=good, repeat=1)
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_rollout_fused_logp_device"):
        env.RolloutFusedDevice(None, T, actions="actor", rec_logp=good)
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_rollout_fused_ex_device"):
        env.RolloutFusedDevice(None, T, actions="actor")


def test_memory_rollout_forwards_rec_logp(gymnet):
    """EpisodeMemory.Rollout hands **rollout_kwargs to RolloutFusedDevice: rec_logp is not one of the streams it records itself"""
    import importlib
    import inspect
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")
    src = inspect.getsource(ve.EpisodeMemory.Rollout)
    assert "**rollout_kwargs)" in src and "rec_logp" not in src
    assert "rec_logp" in inspect.signature(ve.VectorEnv.RolloutFusedDevice).parameters
    assert "logp" in inspect.signature(ve.Actor.Act).parameters and "logp" in inspect.signature(ve.Actor.Step).parameters
