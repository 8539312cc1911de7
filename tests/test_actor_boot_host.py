"""CPU checks of V(terminal observation) on time-limit rows (no GPU).  Fail without the feature: the library exports
gymnet_vecenv_actor_boot_device / gymnet_vecenv_rollout_fused_value_boot_device / gymnet_vecenv_rollout_fused_box_boot_device and the
header, the ctypes mirror, Native.cs, the .hpp and VectorEnv.cs declare them with one arity, at ABI 6; the 20 fused forms of
tests/_actor_boot_cases.py and the stand-alone kernels are in the built library, by mangled name; build.py lists the unit; the profile
lists every form beside the parent's bookkeeping forms; Boot(), Step(boot=) and RolloutFusedDevice(rec_boot=) refuse bad arguments before
any native call and hand good ones across unchanged (against tests/cpp/actor_boot_stub.c built as a shared library); the rollout_body hook
point sits between the scalar record stores and the fused reset.  Pass without it (they test the yardstick): the case table replayed
through the CPU oracle covers every path it is there for, and the NumPy statement of the definition."""
import ctypes
import importlib
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _actor_boot_cases as cases
import _actor_twin as twin
from test_actor_value_host import NoNativeCalls, _bare, _HostTensor, _split_args, _Tensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CALLS = {"gymnet_vecenv_actor_boot_device": 2, "gymnet_vecenv_rollout_fused_value_boot_device": 5, "gymnet_vecenv_rollout_fused_box_boot_device": 5}
BOOT, VALUE_ROLLOUT, BOX_ROLLOUT = 1, 2, 3                        # tests/cpp/actor_boot_stub.c's call ids


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto-reset", "no-reset"])
@pytest.mark.parametrize("name", ["CartPole-v1", "Pendulum-v1", "MountainCar-v0", "Acrobot-v1"])
def test_the_case_table_covers_every_path_on_the_cpu_oracle(name, auto_reset):
    """The table's lengths and goal lanes replayed through the oracle's float32 step (the envs it serves) with random actions and the
    engine's bookkeeping restated in cases.done_bytes: rows with d = 2 (and on the goal envs d = 1 and d = 3) occur, and so do waves with
    every, no and some lanes truncated — the counts the GPU tests assert of their own rec_done."""
    from oracle import capi as oracle
    rng = np.random.default_rng(5)
    for n in (cases.N, cases.N_ATT):
        state = cases.at_the_goal(name, oracle.env_reset(name, 0xAC7, 0, 0, n))
        length = cases.lengths(n)
        assert length.min() == 0 and length.max() == cases.LIMIT - 1
        dones = []
        for t in range(cases.T):
            action = rng.uniform(-2, 2, n).astype(F32) if name == "Pendulum-v1" else rng.integers(0, 2 if name == "CartPole-v1" else 3, n)
            state, _, _, terminated = oracle.env_step(name, state, action, dtype=np.float32)
            done, length = cases.done_bytes(terminated, length, auto_reset)
            if auto_reset and done.any():
                fresh = oracle.env_reset(name, 0xAC7, 0, 1 + t, n)
                state[:, done != 0] = fresh[:, done != 0]
            dones.append(done)
        cov = cases.coverage(np.stack(dones))
        print(f"{name} n={n} auto_reset={auto_reset}: {cov}")
        cases.assert_covered(cov, name)
        if name in cases.GOAL_ENVS:
            assert (dones[0][cases.goal_lanes(n)] & 1).all() and dones[0][69] == 3      # the goal lanes end in the first step; lane 69 both ways


def test_the_coverage_count_itself():
    d = np.zeros((3, 130), np.uint8)
    d[0, :64] = 2                                                  # wave 0 all at step 0
    d[1, 64:70] = 2; d[1, 70] = 3; d[1, 71] = 1                    # wave 1 mixed at step 1, one d = 3 among them, one termination
    d[2, 128:] = 2                                                 # the partial wave (2 lanes) all at step 2
    assert cases.coverage(d) == dict(d1=1, d2=72, d3=1, all=2, none=6, mixed=1)
    with pytest.raises(AssertionError):
        cases.assert_covered(cases.coverage(d[:1]), "Pendulum-v1")  # no mixed wave: the table would not be covering it
    with pytest.raises(AssertionError):
        cases.assert_covered(dict(d1=0, d2=5, d3=1, all=1, none=1, mixed=1), "MountainCar-v0")


def test_the_definition_in_numpy():
    """want_boot over twin.forward: rows 1 .. S-1 of the history and then the terminal observation, on rows with bit 1 only"""
    rng = np.random.default_rng(7)
    name, n, O = "Pendulum-v1", 9, 3
    critic = cases.critic(name, True)
    hist = rng.standard_normal((n, cases.S, O)).astype(F32)
    term = rng.standard_normal((n, O))                              # float64, as a float64 handle's terminal observation arrives
    done = np.array([0, 1, 2, 3, 2, 0, 1, 3, 2], np.uint8)
    got = cases.want_boot(critic, hist, term, done)
    assert got.dtype == F32 and (got.view(np.uint32)[(done & 2) == 0] == 0).all()       # +0.0f, the sign included
    pushed = twin.History(np.zeros((n, O), F32), cases.S)
    pushed.h = hist.copy()
    pushed.push(term.astype(F32), np.zeros(n, np.uint8))            # what Value() would read had the observation been pushed with done = 0
    full = twin.forward(critic[0], critic[1], pushed.x())[0][:, 0]
    assert np.array_equal(got[(done & 2) != 0].view(np.uint32), full[(done & 2) != 0].view(np.uint32)) and (got[done == 3] != 0).all()
    # S = 1: the terminal observation alone
    one = twin.net(np.random.default_rng(1), [O, 5, 1])
    got1 = cases.want_boot(one, hist[:, :1], term, np.full(n, 2, np.uint8))
    assert np.array_equal(got1.view(np.uint32), twin.forward(one[0], one[1], term.astype(F32))[0][:, 0].view(np.uint32))
    # the first history row does not enter
    other = hist.copy(); other[:, 0] += 1.0
    assert np.array_equal(cases.want_boot(critic, other, term, done).view(np.uint32), got.view(np.uint32))


# ---- fail without the feature -----------------------------------------------------------------------------------------------------
def test_the_three_calls_are_exported_and_declared_with_one_arity(gymnet):
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
    for method in ("ActorBoot", "RolloutFusedValueBoot", "RolloutFusedBoxBoot"):
        assert method + "(" in hpp and method + "(" in vcs, method


def _mangled(kernel):
    fn, args = kernel.split("<")
    env, *flags = args.rstrip(">").split(",")
    return f"{len(fn)}{fn}INS_{len(env)}{env}E" + "".join(f"Lb{int(f == 'true')}E" for f in flags) + "E"


def test_the_twenty_forms_are_in_the_built_library(gymnet):
    table = [row["kernel"] for row in cases.FORMS]
    assert len(table) == len(set(table)) == 20 and set(cases.SIBLING) == set(table)
    for row in cases.FORMS:                                       # each row says how to reach its kernel
        fn, env, ar, rec = re.match(r"(\w+)<(\w+),(\w+),(\w+)>", row["kernel"]).groups()
        assert {**cases.DISCRETE, **cases.BOX}[env] == row["env"] and (ar == "true") == row["auto_reset"] and (rec == "true") == row["records"]
        assert fn == ("actor_box_boot_rollout_kernel" if row["box"] else "actor_value_boot_rollout_kernel") and row["box"] == (env in cases.BOX)
    blob = open(gymnet.LIB_PATH, "rb").read()
    for kernel in table:
        assert _mangled(kernel).encode() in blob, kernel
    assert _mangled("actor_value_boot_rollout_kernel<CartPole,true,false>") == "31actor_value_boot_rollout_kernelINS_8CartPoleELb1ELb0EE"
    for standalone in (b"17actor_boot_kernelIfLi2E", b"17actor_boot_kernelIfLi3E", b"17actor_boot_kernelIfLi4E", b"17actor_boot_kernelIfLi6E",
                       b"17actor_boot_kernelIdLi4E"):
        assert standalone in blob, standalone
    assert b"31actor_value_boot_rollout_kernelINS_8PendulumE" not in blob and b"29actor_box_boot_rollout_kernelINS_8CartPoleE" not in blob


def test_the_profile_lists_the_forms_beside_their_parents():
    text = open(os.path.join(ROOT, "profiles", "kernel_resources_actor_boot.txt")).read()
    for name in [row["kernel"] for row in cases.FORMS] + list(cases.SIBLING.values()):
        assert re.search(r"^%s\s+\d+\s+\d+\s+\d+\s+\d+$" % re.escape(name), text, flags=re.M), name       # VGPRs, waves, scratch, LDS
        assert re.search(r"^# %s\s+\d+\s+\d+$" % re.escape(name), text, flags=re.M), name                  # SGPRs, code bytes


def test_the_unit_is_a_build_input_and_the_hook_point_is_where_the_terminal_observation_lives():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    assert "actor_boot.hip" in kernel_resources._BUILD.SOURCES and "actor_boot.hip" in kernel_resources._BUILD.DEPS
    for header in ("actor_box_compose.hpp", "actor_compose_logp.hpp", "actor_net.hpp", "rollout_plan.hpp", "step_kernels.hpp"):
        assert header in kernel_resources._BUILD.DEPS, header
    body = open(os.path.join(kernel_resources.CSRC, "step_kernels.hpp")).read()
    body = body[body.index("void rollout_body("):]
    call = body.index("hook.terminal(t, i0, done, s, o)")
    assert body.index("done[j] |= 2") < body.index("ro.rec_done + t * n") < call < body.index("scalars_recorded:") < body.index("hook.after(t, i0, done, s, o)")
    assert call < body.index("reset_pending_wave<Env, VEC, EXTRAS>(pending, s, a, i0, n, tick, sc)")
    assert "if constexpr (hook_boots<Hook>::value) hook.terminal(" in body                 # compiled in only for a hook that declares BOOTS
    router = open(os.path.join(kernel_resources.CSRC, "actor.hip")).read()
    assert router.count("rec_boot") == 3 and "actor_value_boot_rollout_launch(" in router and "actor_box_boot_rollout_launch(" in router


def test_boot_arguments_are_checked_before_any_native_call(gymnet):
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")
    N, T = 12, 5
    lib = NoNativeCalls()
    good, good_rec = _Tensor((N,)), _Tensor((T, N))
    bad = (_Tensor((N,), "torch.float64"), _Tensor((N,), "torch.int32"), _Tensor((N + 1,)), _Tensor((N, 1)), _Tensor(()), _Tensor((N,), cuda=False),
           _Tensor((N,), contiguous=False), np.zeros(N, F32), 4096)
    bad_rec = (_Tensor((T, N), "torch.float64"), _Tensor((T + 1, N)), _Tensor((T - 1, N)), _Tensor((T, N + 1)), _Tensor((N, T)), _Tensor((T * N,)),
               _Tensor((T, N), cuda=False), _Tensor((T, N), contiguous=False), np.zeros((T, N), F32), 4096)
    # no critic: nothing that asks for a boot reaches the library
    actor = _bare(ve, lib, N, False)._actor
    with pytest.raises(ValueError, match="critic"):
        actor.Boot()
    with pytest.raises(ValueError, match="critic"):
        actor.Boot(out=good)
    with pytest.raises(ValueError, match="critic"):
        actor.Step(0.0, boot=good)
    with pytest.raises(ValueError, match="critic"):
        actor._env.RolloutFusedDevice(None, T, actions="actor", rec_value=good_rec, rec_boot=good_rec)
    for box in (False, True):
        env = _bare(ve, lib, N, box, critic=(8, 16, 1))
        actor = env._actor
        for b in bad:
            with pytest.raises(ValueError):
                actor.Boot(out=b)
            with pytest.raises(ValueError):
                actor.Step(0.0, boot=b)
        with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_boot_device"):      # good arguments do reach the library
            actor.Boot(out=good)
        act = "gymnet_vecenv_actor_box_act_device" if box else "gymnet_vecenv_actor_act_device"
        with pytest.raises(AssertionError, match="native call: " + act):                                # Step: the act call comes first
            actor.Step(0.0, boot=good)
        lp = dict(rec_logd=good_rec) if box else {}
        for rec in bad_rec:
            with pytest.raises(ValueError):
                env.RolloutFusedDevice(None, T, actions="actor", rec_value=good_rec, rec_boot=rec, **lp)
        with pytest.raises(ValueError, match="rec_value"):
            env.RolloutFusedDevice(None, T, actions="actor", rec_boot=good_rec, **lp)
        with pytest.raises(ValueError, match="frame skip"):
            env.RolloutFusedDevice(None, T, actions="actor", rec_value=good_rec, rec_boot=good_rec, repeat=1, **lp)
        for source in ("ring", "sample", "epsilon_greedy"):
            with pytest.raises(ValueError, match="actor"):
                env.RolloutFusedDevice(_Tensor((T, N), "torch.int32"), T, actions=source, rec_value=good_rec, rec_boot=good_rec, **lp)
        call = "gymnet_vecenv_rollout_fused_box_boot_device" if box else "gymnet_vecenv_rollout_fused_value_boot_device"
        old = "gymnet_vecenv_rollout_fused_box_logd_device" if box else "gymnet_vecenv_rollout_fused_value_device"
        for rows in (T, T + 1):
            with pytest.raises(AssertionError, match="native call: " + call):
                env.RolloutFusedDevice(None, T, actions="actor", rec_value=_Tensor((rows, N)), rec_boot=good_rec, **lp)
        with pytest.raises(AssertionError, match="native call: " + old + "$"):                         # ... and without rec_boot the old call
            env.RolloutFusedDevice(None, T, actions="actor", rec_value=good_rec, **lp)
    with pytest.raises(ValueError, match="actor"):
        _bare(ve, lib, N).RolloutFusedDevice(None, T, actions="actor", rec_value=good_rec, rec_boot=good_rec)       # no actor at all
    with pytest.raises(ValueError, match="rec_logd"):                                                   # a Box actor without rec_logd: not built
        _bare(ve, lib, N, True, critic=(8, 16, 1)).RolloutFusedDevice(None, T, actions="actor", rec_value=good_rec, rec_boot=good_rec)


@pytest.fixture(scope="module")
def stub(gymnet, tmp_path_factory):
    """tests/cpp/actor_boot_stub.c as a shared library with the wrapper's prototypes"""
    capi = importlib.import_module(gymnet.__name__ + "._capi")
    so = str(tmp_path_factory.mktemp("boot_stub") / "actor_boot_stub.so")
    r = subprocess.run(["gcc", "-std=gnu11", "-O1", "-Wall", "-Wextra", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "actor_boot_stub.c"), "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lib = ctypes.CDLL(so)
    for name in CALLS:
        getattr(lib, name).restype, getattr(lib, name).argtypes = capi.PROTOTYPES[name]

    class Call(ctypes.Structure):
        _fields_ = [("calls", ctypes.c_int), ("forwarded", ctypes.c_int), ("log", ctypes.c_int * 16), ("epsilon", ctypes.c_float),
                    ("seed", ctypes.c_uint64), ("tick", ctypes.c_uint64), ("steps", ctypes.c_int64), ("action_source", ctypes.c_int32),
                    ("lp_at", ctypes.c_void_p), ("value_at", ctypes.c_void_p), ("boot_at", ctypes.c_void_p)]
    lib.boot_stub_last.restype = ctypes.POINTER(Call)
    lib.boot_stub_setup.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    return lib


def test_the_wrapper_hands_its_arguments_to_the_three_calls_and_raises_on_a_refusal(gymnet, stub):
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")
    capi = importlib.import_module(gymnet.__name__ + "._capi")
    N, T = 12, 5
    stub.boot_stub_clear()
    stub.boot_stub_setup(N, 1, 7)
    last = stub.boot_stub_last().contents
    want_row = np.where(np.arange(N) & 1, 2000.0 + np.arange(N), 0.0).astype(F32)
    want_rec = np.where(np.arange(T * N) & 1, 2000.0 + np.arange(T * N), 0.0).astype(F32)
    for box in (False, True):
        env = _bare(ve, stub, N, box, critic=(8, 16, 1))
        actor = env._actor
        out = _HostTensor(np.full(N, -7.0, F32))
        calls = last.calls
        with pytest.raises(Exception):                               # no step since the push: the library refuses, nothing is written
            actor.Boot(out=out)
        assert last.calls == calls and (out.a == -7.0).all()
        stub.boot_stub_stepped()
        assert actor.Boot(out=out) is out
        assert last.calls == calls + 1 and last.log[calls % 16] == BOOT and last.boot_at == out.data_ptr() and np.array_equal(out.a, want_row)
        stub.boot_stub_pushed()
        # the rollout: three pointers, in their order, with the action stream
        rec_v, rec_b, rec_l = (_HostTensor(np.full((T, N), -7.0, F32)) for _ in range(3))
        lp = dict(rec_logd=rec_l) if box else dict(rec_logp=rec_l)
        env.RolloutFusedDevice(None, T, actions="actor", epsilon=0.75, action_seed=9, action_tick0=100, rec_value=rec_v, rec_boot=rec_b, **lp)
        assert last.log[(calls + 1) % 16] == (BOX_ROLLOUT if box else VALUE_ROLLOUT) and last.forwarded == 0
        assert (last.steps, last.action_source, last.epsilon, last.seed, last.tick) == (T, capi.ACTIONS_ACTOR, 0.75, 9, 100)
        assert (last.lp_at, last.value_at, last.boot_at) == (rec_l.data_ptr(), rec_v.data_ptr(), rec_b.data_ptr())
        assert np.array_equal(rec_b.a.ravel(), want_rec) and np.array_equal(rec_v.a.ravel(), np.arange(T * N, dtype=F32))
        assert np.array_equal(rec_l.a.ravel(), -np.arange(T * N, dtype=F32))
        if not box:                                                  # without rec_logp a null pointer crosses
            rec_b.a.fill(-7.0)
            env.RolloutFusedDevice(None, T, actions="actor", rec_value=rec_v, rec_boot=rec_b)
            assert last.lp_at is None and np.array_equal(rec_b.a.ravel(), want_rec)
        # a refusal of the library raises and writes nothing: no time limit
        stub.boot_stub_setup(N, 1, 0)
        rec_b.a.fill(-7.0); rec_v.a.fill(-7.0)
        calls = last.calls
        with pytest.raises(Exception):
            env.RolloutFusedDevice(None, T, actions="actor", rec_value=rec_v, rec_boot=rec_b, **lp)
        assert last.calls == calls and (rec_b.a == -7.0).all() and (rec_v.a == -7.0).all()
        stub.boot_stub_setup(N, 1, 7)


def test_memory_rollout_forwards_rec_boot(gymnet):
    """EpisodeMemory.Rollout hands **rollout_kwargs to RolloutFusedDevice: rec_boot is not one of the streams it records itself"""
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")
    src = inspect.getsource(ve.EpisodeMemory.Rollout)
    assert "**rollout_kwargs)" in src and "rec_boot" not in src
    assert "rec_boot" in inspect.signature(ve.VectorEnv.RolloutFusedDevice).parameters
    assert "boot" in inspect.signature(ve.Actor.Step).parameters and callable(ve.Actor.Boot)
