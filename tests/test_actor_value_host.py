"""CPU checks of the critic a configured actor carries (no GPU).  Every test fails without the feature: the library exports the five calls
(gymnet_vecenv_actor_critic_config / _actor_critic_load_device / _actor_value_device / _actor_act_value_device and
gymnet_vecenv_rollout_fused_value_device) and the header, the ctypes mirror, Native.cs, the .hpp and VectorEnv.cs declare them with one
arity, at ABI 6; actor_value.hip compiles the 18 fused forms of tests/_actor_logp_forms.py under its own kernel name and the four
stand-alone kernels, nothing else, each at its logp sibling's waves per SIMD and LDS; build.py lists the unit and the shared header;
the profile lists every compiled kernel; SetCritic / LoadCritic / Value / Act(value=) / Step(value=) / RolloutFusedDevice(rec_value=)
refuse wrong shapes, dtypes, devices, a Box actor, a missing critic and a critic whose first or last width is wrong before any native
call; and against the C stub (tests/cpp/actor_value_stub.c, built as a shared library and handed to the wrapper in the library's place)
rec_value with T + 1 rows issues the rollout and then the value call into row T, with T rows the rollout alone."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CALLS = {"gymnet_vecenv_actor_critic_config": 5, "gymnet_vecenv_actor_critic_load_device": 3, "gymnet_vecenv_actor_value_device": 2,
         "gymnet_vecenv_actor_act_value_device": 8, "gymnet_vecenv_rollout_fused_value_device": 4}
VALUE_KERNELS = tuple(f"actor_value_kernel<{o}>" for o in (2, 3, 4, 6))
ROLLOUT = {row["kernel"]: row["kernel"].replace("actor_logp_rollout_kernel", "actor_value_rollout_kernel") for row in forms.FORMS}
CONFIG, LOAD, VALUE, ACT, ROLLOUT_CALL = 1, 2, 3, 4, 5              # tests/cpp/actor_value_stub.c's call ids


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


def test_the_five_calls_are_exported_and_declared_with_one_arity(gymnet):
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
    for method in ("ConfigureActorCritic", "LoadActorCriticWeights", "ActorValue", "ActorActValue", "RolloutFusedValue"):
        assert method + "(" in hpp and method + "(" in vcs, method


@pytest.fixture(scope="module")
def unit_kernels():
    """({kernel name: resources} of actor_value.hip, the same of actor_logp.hip), both compiled to gfx950 assembly with the product's flags
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
            return tuple(ex.map(compile_unit, ("actor_value", "actor_logp")))


@pytest.mark.timeout(900)
def test_the_unit_compiles_the_18_forms_and_the_four_value_kernels(unit_kernels):
    kernels, siblings = unit_kernels
    compiled = sorted(n for n in kernels if n.startswith("actor_value_rollout_kernel<"))
    assert compiled == sorted(ROLLOUT.values()) and len(set(compiled)) == 18
    assert set(VALUE_KERNELS) <= set(kernels)
    assert len(kernels) == 22                                     # one kernel per form, with and without rec_logp; nothing else
    # against the actor_logp.hip sibling: the waves per SIMD the launch bounds ask for, and equal LDS.  Scratch is listed, not asserted:
    # the lean CartPole forms sit at the 168-VGPR bound (profiles/kernel_resources_actor_value.txt says which use scratch and how much)
    for logp_name, name in ROLLOUT.items():
        k, s = kernels[name], siblings[logp_name]
        print(f"{name:64s} VGPRs {k['vgpr']:3d} (logp {s['vgpr']:3d})  waves {k['occupancy']} ({s['occupancy']})  scratch {k['scratch']} ({s['scratch']})  "
              f"LDS {k['lds']} ({s['lds']})")
        assert k["occupancy"] >= s["occupancy"] and k["occupancy"] >= 2, (name, k, s)
        assert k["lds"] == s["lds"], (name, k, s)
    for name in VALUE_KERNELS:
        assert kernels[name]["scratch"] == 0 and kernels[name]["lds"] == 0 and kernels[name]["occupancy"] >= 3, (name, kernels[name])


def test_the_profile_lists_the_compiled_kernels():
    text = open(os.path.join(ROOT, "profiles", "kernel_resources_actor_value.txt")).read()
    for name in list(ROLLOUT.values()) + list(VALUE_KERNELS) + list(ROLLOUT):          # ... beside the logp forms' figures
        assert re.search(r"^%s\s+\d+\s+\d+\s+\d+\s+\d+$" % re.escape(name), text, flags=re.M), name


def test_the_unit_is_a_build_input():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    assert "actor_value.hip" in kernel_resources._BUILD.SOURCES and "actor_value.hip" in kernel_resources._BUILD.DEPS
    assert "actor_compose_logp.hpp" in kernel_resources._BUILD.DEPS
    csrc = os.path.join(ROOT, "gym.net_amd", "csrc")
    for unit in ("actor_logp.hip", "actor_value.hip"):            # one composition, shared: neither unit keeps a copy
        src = open(os.path.join(csrc, unit)).read()
        assert '#include "actor_compose_logp.hpp"' in src and "int32_t compose_one_logp(" not in src, unit
    assert "int32_t compose_one_logp(" in open(os.path.join(csrc, "actor_compose_logp.hpp")).read()


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


def _pairs(widths, rng=None):
    rng = rng or np.random.default_rng(3)
    return [(rng.standard_normal((widths[k + 1], widths[k])).astype(F32), rng.standard_normal(widths[k + 1]).astype(F32)) for k in range(len(widths) - 1)]


def _bare(ve, lib, N, actor_is_box=None, critic=None):
    env = ve.VectorEnv.__new__(ve.VectorEnv)
    env.__dict__.update(_lib=lib, _h=1, _owns_handle=False, NumberOfEnvironments=N, Device=0)
    if actor_is_box is not None:
        o = ve.Actor.__new__(ve.Actor)
        o.__dict__.update(IsBox=actor_is_box, _lib=lib, _h=1, _env=env, _out=_Tensor((N,), "torch.int32"), Widths=(8, 16, 2), Count=0,
                          CriticWidths=critic, CriticCount=0 if critic is None else sum(critic[k + 1] * critic[k] + critic[k + 1] for k in range(len(critic) - 1)))
        env._actor = o
    return env


def test_value_arguments_are_checked_before_any_native_call(gymnet):
    import importlib
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")
    N, T = 12, 5
    lib = NoNativeCalls()
    out = _Tensor((N,), "torch.int32")
    good = _Tensor((N,))
    bad = (_Tensor((N,), "torch.float64"), _Tensor((N,), "torch.int32"), _Tensor((N + 1,)), _Tensor((N, 1)), _Tensor((1, N)), _Tensor(()),
           _Tensor((N,), cuda=False), _Tensor((N,), contiguous=False), np.zeros(N, F32), 4096, [0.0] * N)
    # a critic whose first or last width is wrong, a network that is none
    actor = _bare(ve, lib, N, False)._actor
    for widths in ([9, 16, 1], [4, 1], [8, 16, 2], [8, 16, 7, 3]):
        with pytest.raises(ValueError, match="critic"):
            actor.SetCritic(_pairs(widths))
    with pytest.raises(ValueError):
        actor.SetCritic([])
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_critic_config"):         # good ones reach the library ...
        actor.SetCritic(_pairs([8, 13, 7, 1]))
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_critic_config"):         # ... and so does the removal
        actor.SetCritic(None)
    assert actor.CriticWidths is None
    # no critic: nothing that asks for a value reaches the library
    with pytest.raises(ValueError, match="critic"):
        actor.LoadCritic(_pairs([8, 16, 1]))
    with pytest.raises(ValueError, match="critic"):
        actor.Value(out=good)
    with pytest.raises(ValueError, match="critic"):
        actor.Act(0.0, out=out, value=good)
    with pytest.raises(ValueError, match="critic"):
        actor.Step(0.0, value=good)
    with pytest.raises(ValueError, match="critic"):
        actor._env.RolloutFusedDevice(None, T, actions="actor", rec_value=_Tensor((T, N)))
    # a critic of widths (8, 16, 1)
    env = _bare(ve, lib, N, False, critic=(8, 16, 1))
    actor = env._actor
    for widths in ([8, 15, 1], [8, 16, 4, 1], [8, 1]):
        with pytest.raises(ValueError, match="widths"):
            actor.LoadCritic(_pairs(widths))
    with pytest.raises(ValueError, match="critic"):
        actor.LoadCritic(_pairs([9, 16, 1]))
    for value in bad:
        with pytest.raises(ValueError):
            actor.Value(out=value)
        with pytest.raises(ValueError):
            actor.Act(0.0, out=out, value=value)
        with pytest.raises(ValueError):
            actor.Step(0.0, value=value)
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_value_device"):
        actor.Value(out=good)
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_act_value_device"):
        actor.Act(0.0, out=out, value=good)
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_act_value_device"):
        actor.Act(0.0, out=out, logp=_Tensor((N,)), value=good)
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_act_value_device"):
        actor.Step(0.0, repeat=2, value=good)
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_act_logp_device"):       # without value the old calls
        actor.Act(0.0, out=out, logp=_Tensor((N,)))
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_act_device"):
        actor.Act(0.0, out=out)
    # a Box actor: Value serves it, Act(value=) / Step(value=) / rec_value do not
    box = _bare(ve, lib, N, True, critic=(8, 16, 1))
    with pytest.raises(ValueError, match="Box"):
        box._actor.Act(0.0, out=_Tensor((N,)), value=good)
    with pytest.raises(ValueError, match="Box"):
        box._actor.Step(0.0, value=good)
    with pytest.raises(ValueError, match="Box"):
        box.RolloutFusedDevice(None, T, actions="actor", rec_value=_Tensor((T, N)))
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_value_device"):
        box._actor.Value(out=good)
    # the fused rollout's rec_value
    with pytest.raises(ValueError, match="actor"):
        _bare(ve, lib, N).RolloutFusedDevice(None, T, actions="actor", rec_value=_Tensor((T, N)))       # no actor at all
    for source in ("ring", "sample", "epsilon_greedy"):
        with pytest.raises(ValueError, match="actor"):
            env.RolloutFusedDevice(_Tensor((T, N), "torch.int32"), T, actions=source, rec_value=_Tensor((T, N)))
    for rec in (_Tensor((T, N), "torch.float64"), _Tensor((T, N), "torch.float16"), _Tensor((T + 2, N)), _Tensor((T - 1, N)), _Tensor((T, N + 1)),
                _Tensor((T + 1, N + 1)), _Tensor((N, T)), _Tensor((T * N,)), _Tensor((T, N), cuda=False), _Tensor((T + 1, N), cuda=False),
                _Tensor((T, N), contiguous=False), np.zeros((T, N), F32), 4096):
        with pytest.raises(ValueError):
            env.RolloutFusedDevice(None, T, actions="actor", rec_value=rec)
    with pytest.raises(ValueError):
        env.RolloutFusedDevice(None, T, actions="actor", rec_value=_Tensor((T, N)), repeat=1)
    with pytest.raises(ValueError):                                                                      # rec_logp is still checked beside it
        env.RolloutFusedDevice(None, T, actions="actor", rec_value=_Tensor((T, N)), rec_logp=_Tensor((T + 1, N)))
    for rows in (T, T + 1):
        with pytest.raises(AssertionError, match="native call: gymnet_vecenv_rollout_fused_value_device"):
            env.RolloutFusedDevice(None, T, actions="actor", rec_value=_Tensor((rows, N)))
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_rollout_fused_logp_device"):
        env.RolloutFusedDevice(None, T, actions="actor", rec_logp=_Tensor((T, N)))
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_rollout_fused_ex_device"):
        env.RolloutFusedDevice(None, T, actions="actor")


class _HostTensor:
    """a numpy array behind the attributes the wrapper reads of a device tensor: the stub writes host memory"""

    def __init__(self, array):
        self.a = array
        self.shape, self.dtype, self.is_cuda = array.shape, "torch." + array.dtype.name, True

    def data_ptr(self):
        return self.a.ctypes.data

    def is_contiguous(self):
        return True


@pytest.fixture(scope="module")
def stub(gymnet, tmp_path_factory):
    """tests/cpp/actor_value_stub.c as a shared library with the wrapper's prototypes"""
    import importlib
    capi = importlib.import_module(gymnet.__name__ + "._capi")
    so = str(tmp_path_factory.mktemp("value_stub") / "actor_value_stub.so")
    r = subprocess.run(["gcc", "-std=gnu11", "-O1", "-Wall", "-Wextra", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "actor_value_stub.c"), "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lib = ctypes.CDLL(so)
    for name in CALLS:
        getattr(lib, name).restype, getattr(lib, name).argtypes = capi.PROTOTYPES[name]

    class Call(ctypes.Structure):
        _fields_ = [("calls", ctypes.c_int), ("forwarded", ctypes.c_int), ("log", ctypes.c_int * 16), ("num_layers", ctypes.c_int32),
                    ("count", ctypes.c_int64), ("weight_sum", ctypes.c_float), ("epsilon", ctypes.c_float), ("seed", ctypes.c_uint64),
                    ("tick", ctypes.c_uint64), ("steps", ctypes.c_int64), ("action_source", ctypes.c_int32), ("value_at", ctypes.c_void_p),
                    ("has_critic", ctypes.c_int)]
    lib.value_stub_last.restype = ctypes.POINTER(Call)
    lib.value_stub_lanes.argtypes = [ctypes.c_int64, ctypes.c_int32]
    return lib


def test_rec_value_with_one_more_row_issues_the_rollout_and_then_the_value_call(gymnet, stub):
    import importlib
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")
    capi = importlib.import_module(gymnet.__name__ + "._capi")
    N, T = 12, 5
    stub.value_stub_clear()
    stub.value_stub_lanes(N, 8)
    last = stub.value_stub_last().contents
    env = _bare(ve, stub, N, False)
    actor = env._actor
    pairs = _pairs([8, 13, 7, 1])
    actor.SetCritic(pairs)                                           # through the stub: widths and weights cross, and the wrapper remembers them
    count = sum(w.size + b.size for w, b in pairs)
    assert list(last.log[:last.calls]) == [CONFIG] and last.num_layers == 3 and last.count == count == actor.CriticCount
    assert actor.CriticWidths == (8, 13, 7, 1)
    assert np.isclose(last.weight_sum, sum(float(w.sum()) + float(b.sum()) for w, b in pairs), atol=1e-3)
    value = _HostTensor(np.full(N, -7.0, F32))
    assert actor.Value(out=value) is value
    assert list(last.log[:last.calls]) == [CONFIG, VALUE] and last.value_at == value.data_ptr()
    assert np.array_equal(value.a, 1000.0 + np.arange(N, dtype=F32))
    # T + 1 rows: the rollout, then the value call into row T
    rec = _HostTensor(np.full((T + 1, N), -7.0, F32))
    logp = _HostTensor(np.full((T, N), 7.0, F32))
    env.RolloutFusedDevice(None, T, actions="actor", epsilon=0.75, action_seed=9, action_tick0=100, rec_logp=logp, rec_value=rec)
    assert list(last.log[:last.calls]) == [CONFIG, VALUE, ROLLOUT_CALL, VALUE]
    assert (last.steps, last.action_source, last.epsilon, last.seed, last.tick) == (T, capi.ACTIONS_ACTOR, 0.75, 9, 100)
    assert last.value_at == rec.data_ptr() + 4 * T * N
    assert np.array_equal(rec.a[:T].ravel(), np.arange(T * N, dtype=F32)) and np.array_equal(rec.a[T], 1000.0 + np.arange(N, dtype=F32))
    assert np.array_equal(logp.a.ravel(), -np.arange(T * N, dtype=F32))
    # T rows: the rollout alone, and without rec_logp a null pointer crosses
    rec = _HostTensor(np.full((T, N), -7.0, F32))
    logp.a.fill(7.0)
    env.RolloutFusedDevice(None, T, actions="actor", rec_value=rec)
    assert list(last.log[:last.calls]) == [CONFIG, VALUE, ROLLOUT_CALL, VALUE, ROLLOUT_CALL] and last.forwarded == 0
    assert np.array_equal(rec.a.ravel(), np.arange(T * N, dtype=F32)) and (logp.a == 7.0).all()
    # a refused rollout is not followed by a value call
    actor.SetCritic(None)
    actor.CriticWidths = (8, 13, 7, 1)                               # (the wrapper believes in a critic the library has dropped)
    rec = _HostTensor(np.full((T + 1, N), -7.0, F32))
    calls = last.calls
    with pytest.raises(Exception):
        env.RolloutFusedDevice(None, T, actions="actor", rec_value=rec)
    assert last.calls == calls and (rec.a == -7.0).all()


def test_memory_rollout_forwards_rec_value(gymnet):
    """EpisodeMemory.Rollout hands **rollout_kwargs to RolloutFusedDevice: rec_value is not one of the streams it records itself"""
    import importlib
    import inspect
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")
    src = inspect.getsource(ve.EpisodeMemory.Rollout)
    assert "**rollout_kwargs)" in src and "rec_value" not in src
    assert "rec_value" in inspect.signature(ve.VectorEnv.RolloutFusedDevice).parameters
    assert "value" in inspect.signature(ve.Actor.Act).parameters and "value" in inspect.signature(ve.Actor.Step).parameters
    for method in ("SetCritic", "LoadCritic", "Value"):
        assert callable(getattr(ve.Actor, method))
