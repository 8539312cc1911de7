"""CPU checks of the log-density a Box actor records (no GPU).  Fail without the feature: the library exports
gymnet_vecenv_actor_box_act_logd_device / gymnet_vecenv_rollout_fused_box_logd_device and the header, the ctypes mirror, Native.cs, the
.hpp and VectorEnv.cs declare them with one arity, at ABI 6; the recipe table of tests/_actor_box_logd_forms.py equals the
actor_box_logd_rollout_kernel forms in actor_box_logd.hip's gfx950 assembly, by name, the two act kernels exist, the unit compiles 14
kernels, and every one of them keeps its actor_box_policy.hip sibling's waves per SIMD and LDS with no scratch; build.py lists the unit
and its header; Act(logd=), Step(logd=) and RolloutFusedDevice(rec_logd=) refuse a Discrete actor, a wrong dtype / shape / device, a frame
skip, and rec_value without rec_logd on a Box actor before any native call; the profile lists every compiled kernel.  Passes without it
(it tests the yardstick): the twin against the float64 closed form."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import _actor_box_logd_forms as forms
import _actor_box_logd_twin as dtwin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CALLS = {"gymnet_vecenv_actor_box_act_logd_device": 7, "gymnet_vecenv_rollout_fused_box_logd_device": 4}


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


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
def test_the_twin_against_the_float64_closed_form():
    """Random (a, g) inside both envs' bounds at the four sigmas, against -d^2 / 2 - ln sigma - ln(2 pi) / 2 in float64 of the same float32
    inputs, within 2^-21 * max(1, d^2, |c|).  The derivation: three roundings reach d (the difference, inv_sigma, the product), each
    2^-24 relative, doubled by the square and halved by the 1/2: 3 * 2^-24 * d^2; the rounding of h * d is none (the fmaf keeps the exact
    product); c carries one rounding, 2^-24 |c|, and the result one more, 2^-24 * (d^2 / 2 + |c|) at most: 2^-24 * (3.5 d^2 + 2 |c|) in
    all, below 2^-21 * max(1, d^2, |c|).  A condition, not a measurement; the worst ratio is printed."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for name, (low, high) in forms.BOUNDS.items():
        for sigma in dtwin.SIGMAS:
            a, g = (rng.uniform(low, high, 150000).astype(F32) for _ in range(2))
            a[:1000] = g[:1000]                                              # greedy lanes
            a[1000:2000] = F32(high); a[2000:3000] = F32(low)                # the clamp bit
            got = dtwin.logd(a, g, sigma)
            want, d2 = dtwin.logd64(a, g, sigma)
            c = float(dtwin.constants(sigma)[1])
            ratio = np.abs(got.astype(np.float64) - want) / (2.0 ** -21 * np.maximum(1.0, np.maximum(d2, abs(c))))
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (name, sigma, int(np.argmax(ratio)))
            assert (got[:1000].view(np.uint32) == dtwin.constants(sigma)[1].view(np.uint32)).all()      # a == g: exactly c
    print(f"twin against the float64 closed form over {2 * 4 * 150000} draws: worst error / bound {worst:.3f}")


def test_the_twins_constants_and_edges():
    inv, c = dtwin.constants(0.5)
    assert inv == F32(2.0) and c == F32(-0.2257913526447274)                 # 1 / 0.5; ln 2 - ln(2 pi) / 2
    inv, c = dtwin.constants(0.25)
    assert inv == F32(4.0) and c == F32(0.4673558279152179)                  # ln 4 - ln(2 pi) / 2
    # d = (1.5 - 0.5) * 4 = 4: -8 + c, one rounding
    assert dtwin.logd([1.5], [0.5], 0.25)[0] == F32(-8.0 + np.float64(c))
    with np.errstate(all="ignore"):
        assert np.isnan(dtwin.logd([0.0], [np.nan], 0.5)[0])                 # a NaN g gives a NaN
        assert dtwin.logd([3e38], [-3e38], 0.5)[0] == -np.inf                # an overflowing d^2 gives -inf
    assert dtwin.logd([-0.0], [0.0], 0.3)[0].view(np.uint32) == dtwin.constants(0.3)[1].view(np.uint32)


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
    for method in ("BoxActorActLogd", "RolloutFusedBoxLogd"):
        assert method + "(" in hpp and method + "(" in vcs, method


@pytest.fixture(scope="module")
def unit_kernels():
    """{kernel name: resources} of actor_box_logd.hip and of actor_box_policy.hip, both compiled to gfx950 assembly with the product's flags
    (tools/kernel_resources.py)"""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    return kernel_resources.collect(["actor_box_logd.hip"]), kernel_resources.collect(["actor_box_policy.hip"])


@pytest.mark.timeout(900)
def test_forms_table_names_every_compiled_logd_rollout_kernel(unit_kernels):
    kernels, _ = unit_kernels
    compiled = sorted(n for n in kernels if n.startswith("actor_box_logd_rollout_kernel<"))
    table = sorted(row["kernel"] for row in forms.FORMS)
    assert len(table) == len(set(table)) == 12
    assert compiled == table, (sorted(set(compiled) - set(table)), sorted(set(table) - set(compiled)))
    for row in forms.FORMS:                                       # each row says how to reach its kernel
        env, ar, extras, records = re.match(r"actor_box_logd_rollout_kernel<(\w+),(\w+),(\w+),(\w+)>", row["kernel"]).groups()
        assert forms.ENVS[env] == row["env"] and (ar == "true") == row["auto_reset"]
        assert (extras == "true", records == "true") == forms.SHAPES[row["shape"]]
    assert set(forms.ACT_KERNELS) <= set(kernels)
    assert len(kernels) == 14                                     # the unit compiles nothing else


@pytest.mark.timeout(900)
def test_logd_kernels_keep_their_siblings_occupancy_and_lds_without_scratch(unit_kernels):
    """against the actor_box_policy.hip sibling: waves per SIMD not below it, equal LDS, no scratch (the sibling has none).  The VGPR
    counts are listed (and kept in profiles/kernel_resources_actor_box_logd.txt), not asserted beyond what the occupancy implies."""
    kernels, siblings = unit_kernels
    for n in sorted(kernels):
        k, s = kernels[n], siblings[forms.SIBLING[n]]
        print(f"{n:72s} VGPRs {k['vgpr']:3d} (sibling {s['vgpr']:3d})  waves {k['occupancy']} ({s['occupancy']})  scratch {k['scratch']} ({s['scratch']})  "
              f"LDS {k['lds']} ({s['lds']})")
        assert k["occupancy"] >= s["occupancy"] and k["occupancy"] >= 2, (n, k, s)
        assert k["lds"] == s["lds"], (n, k, s)
        assert k["scratch"] == s["scratch"] == 0, (n, k, s)


def test_the_profile_lists_the_compiled_kernels():
    text = open(os.path.join(ROOT, "profiles", "kernel_resources_actor_box_logd.txt")).read()
    for name in [row["kernel"] for row in forms.FORMS] + list(forms.ACT_KERNELS):
        assert re.search(r"^%s\s+\d+\s+\d+\s+\d+\s+\d+$" % re.escape(name), text, flags=re.M), name


def test_the_unit_is_a_build_input():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    assert "actor_box_logd.hip" in kernel_resources._BUILD.SOURCES and "actor_box_logd.hip" in kernel_resources._BUILD.DEPS
    for header in ("actor_box_compose.hpp", "actor_net.hpp", "rollout_plan.hpp"):
        assert header in kernel_resources._BUILD.DEPS, header
    policy = open(os.path.join(kernel_resources.CSRC, "actor_box_policy.hip")).read()
    logd = open(os.path.join(kernel_resources.CSRC, "actor_box_logd.hip")).read()
    for unit in (policy, logd):                                   # both units run the one composition
        assert '#include "actor_box_compose.hpp"' in unit and "policy_compose_one(" not in unit and "policy_choose<O>(" in unit


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


def test_logd_arguments_are_checked_before_any_native_call(gymnet):
    import importlib
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")
    N, T = 12, 5

    def bare_env(actor_is_box=None, critic=None):
        env = ve.VectorEnv.__new__(ve.VectorEnv)
        env.__dict__.update(_lib=NoNativeCalls(), _h=1, _owns_handle=False, NumberOfEnvironments=N, Device=0)
        if actor_is_box is not None:
            env._actor = bare_actor(actor_is_box, env, critic)
        return env

    def bare_actor(is_box, env=None, critic=None):
        o = ve.Actor.__new__(ve.Actor)
        o.__dict__.update(IsBox=is_box, _lib=NoNativeCalls(), _h=1, _env=env or bare_env(), _out=_Tensor((N,)), CriticWidths=critic)
        return o

    out = _Tensor((N,))
    with pytest.raises(ValueError, match="Discrete"):
        bare_actor(False).Act(0.0, out=out, logd=_Tensor((N,)))
    with pytest.raises(ValueError, match="Discrete"):
        bare_actor(False).Step(0.0, logd=_Tensor((N,)))
    actor = bare_actor(True)
    bad = (_Tensor((N,), "torch.float64"), _Tensor((N,), "torch.int32"), _Tensor((N + 1,)), _Tensor((N, 1)), _Tensor((1, N)), _Tensor(()),
           _Tensor((N,), cuda=False), _Tensor((N,), contiguous=False), np.zeros(N, F32), 4096, [0.0] * N)
    for logd in bad:
        with pytest.raises(ValueError):
            actor.Act(0.0, out=out, logd=logd)
        with pytest.raises(ValueError):
            actor.Step(0.0, logd=logd)
    with pytest.raises(ValueError, match="Box"):                                                       # the old names keep refusing a Box actor
        actor.Act(0.0, out=out, logp=_Tensor((N,)))
    with pytest.raises(ValueError, match="Box"):
        actor.Act(0.0, out=out, value=_Tensor((N,)))
    with pytest.raises(ValueError, match="Box"):
        actor.Act(0.0, out=out, logd=_Tensor((N,)), value=_Tensor((N,)))                               # no Act(value=) for Box, with logd either
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_box_act_logd_device"):  # good arguments do reach the library
        actor.Act(0.0, out=out, logd=_Tensor((N,)))
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_box_act_logd_device"):
        actor.Step(0.0, repeat=2, logd=_Tensor((N,)))
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_box_act_device"):       # ... and without logd the old call
        actor.Act(0.0, out=out)
    good = _Tensor((T, N))
    with pytest.raises(ValueError, match="Discrete"):
        bare_env(False).RolloutFusedDevice(None, T, actions="actor", rec_logd=good)
    with pytest.raises(ValueError, match="actor"):
        bare_env().RolloutFusedDevice(None, T, actions="actor", rec_logd=good)                          # no actor at all
    env = bare_env(True)
    for source in ("ring", "sample", "epsilon_greedy"):
        with pytest.raises(ValueError, match="actor"):
            env.RolloutFusedDevice(_Tensor((T, N)), T, actions=source, rec_logd=good)
    for rec in (_Tensor((T, N), "torch.float64"), _Tensor((T, N), "torch.float16"), _Tensor((T + 1, N)), _Tensor((T, N + 1)), _Tensor((N, T)),
                _Tensor((T * N,)), _Tensor((T, N), cuda=False), _Tensor((T, N), contiguous=False), np.zeros((T, N), F32), 4096):
        with pytest.raises(ValueError):
            env.RolloutFusedDevice(None, T, actions="actor", rec_logd=rec)
    with pytest.raises(ValueError, match="frame skip"):
        env.RolloutFusedDevice(None, T, actions="actor", rec_logd=good, repeat=1)
    with pytest.raises(ValueError, match="Box"):
        env.RolloutFusedDevice(None, T, actions="actor", rec_logd=good, rec_logp=good)
    with pytest.raises(ValueError, match="Box.*rec_logd|rec_logd.*Box"):                                # rec_value alone on a Box actor
        bare_env(True, critic=(6, 16, 1)).RolloutFusedDevice(None, T, actions="actor", rec_value=good)
    with pytest.raises(ValueError, match="critic"):
        env.RolloutFusedDevice(None, T, actions="actor", rec_logd=good, rec_value=good)
    with_critic = bare_env(True, critic=(6, 16, 1))
    for rec in (_Tensor((T + 2, N)), _Tensor((T, N + 1)), _Tensor((T, N), "torch.float64"), _Tensor((T + 1, N), cuda=False), np.zeros((T, N), F32)):
        with pytest.raises(ValueError):
            with_critic.RolloutFusedDevice(None, T, actions="actor", rec_logd=good, rec_value=rec)
    for rows in (T, T + 1):
        with pytest.raises(AssertionError, match="native call: gymnet_vecenv_rollout_fused_box_logd_device"):
            with_critic.RolloutFusedDevice(None, T, actions="actor", rec_logd=good, rec_value=_Tensor((rows, N)))
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_rollout_fused_box_logd_device"):
        env.RolloutFusedDevice(None, T, actions="actor", rec_logd=good)
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_rollout_fused_ex_device"):
        env.RolloutFusedDevice(None, T, actions="actor")


def test_memory_rollout_forwards_rec_logd(gymnet):
    """EpisodeMemory.Rollout hands **rollout_kwargs to RolloutFusedDevice: rec_logd is not one of the streams it records itself"""
    import importlib
    import inspect
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")
    src = inspect.getsource(ve.EpisodeMemory.Rollout)
    assert "**rollout_kwargs)" in src and "rec_logd" not in src
    assert "rec_logd" in inspect.signature(ve.VectorEnv.RolloutFusedDevice).parameters
    assert "logd" in inspect.signature(ve.Actor.Act).parameters and "logd" in inspect.signature(ve.Actor.Step).parameters
