"""CPU checks of frame skip (no GPU).  Fail without the feature: the library exports the three calls and the ctypes mirror, the header and
Native.cs agree on their arity; the recipe table of tests/_action_repeat_forms.py equals the repeat_rollout_kernel forms in
action_repeat.hip's gfx950 assembly, by name; no kernel of the unit uses scratch; the Python wrappers refuse repeat = -1 and 256 before
any native call.  Pass without it (they test the test's own yardstick): the NumPy model of tests/_action_repeat_model.py on hand-worked
CartPole and MountainCar sequences — a lane that terminates at sub-step 1 of 4, a lane that truncates at sub-step 0, a -0.0 first reward."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _action_repeat_forms as forms
import _action_repeat_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CALLS = {"gymnet_vecenv_step_repeat_device": 3, "gymnet_vecenv_step_repeat": 6, "gymnet_vecenv_rollout_repeat_device": 3}


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


# ---- fail without the feature -----------------------------------------------------------------------------------------------------
def test_the_three_calls_are_exported_and_declared_with_one_arity(gymnet):
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
    hpp = open(os.path.join(ROOT, "include", "gymnet_amd.hpp")).read()
    vcs = open(os.path.join(ROOT, "gym.net_amd", "csharp", "VectorEnv.cs")).read()
    for name in CALLS:
        assert name + "(" in hpp and "Native." + name + "(" in vcs, name


@pytest.fixture(scope="module")
def unit_kernels():
    """{kernel name: resources} of action_repeat.hip compiled to gfx950 assembly with the product's flags (tools/kernel_resources.py)"""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    assert "action_repeat.hip" in kernel_resources._BUILD.SOURCES and "action_repeat.hip" in kernel_resources._BUILD.DEPS
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "action_repeat.s")
        r = subprocess.run([kernel_resources.HIPCC] + kernel_resources.FLAGS + [os.path.join(kernel_resources.CSRC, "action_repeat.hip"), "-o", out],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return kernel_resources.kernels(out)


@pytest.mark.timeout(900)
def test_forms_table_names_every_compiled_kernel_of_the_unit(unit_kernels):
    compiled = sorted(unit_kernels)
    table = sorted(row["kernel"] for row in forms.FORMS)
    assert len(table) == len(set(table)) == 72
    assert compiled == table, (sorted(set(compiled) - set(table)), sorted(set(table) - set(compiled)))
    for row in forms.FORMS:                                       # each row says how to reach its kernel
        env, ar, extras, sample, records = re.match(r"repeat_rollout_kernel<(\w+),(\w+),(\w+),(\w+),(\w+)>", row["kernel"]).groups()
        assert forms.ENVS[env] == (row["env"], row["dtype"]) and (ar == "true") == row["auto_reset"]
        assert (extras == "true", records == "true") == forms.SHAPES[row["shape"]] and (sample == "true") == forms.SOURCES[row["actions"]]


@pytest.mark.timeout(900)
def test_no_kernel_of_the_unit_uses_scratch(unit_kernels):
    assert unit_kernels
    for n in sorted(unit_kernels):
        assert unit_kernels[n]["scratch"] == 0, (n, unit_kernels[n])


@pytest.mark.parametrize("bad", [-1, 256])
def test_wrappers_refuse_a_repeat_out_of_range_before_any_native_call(gymnet, bad):
    import importlib
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")

    class NoNativeCalls:
        def __getattr__(self, name):
            raise AssertionError("native call: " + name)

    def bare(cls, **attrs):
        o = cls.__new__(cls)
        o.__dict__.update(attrs)
        return o
    env = bare(ve.VectorEnv, _lib=NoNativeCalls(), _h=None, NumberOfEnvironments=4, _adtype=np.int32, _dtype=np.dtype(np.float32), ObsDim=4)
    a = np.zeros(4, np.int32)
    for call in (lambda: env.StepRepeatDevice(0, bad), lambda: env.StepRepeat(a, bad), lambda: env.RolloutFusedDevice(0, 1, repeat=bad),
                 lambda: bare(ve.PixelFrameStack, _env=env, _lib=NoNativeCalls(), _h=1).Step(0, repeat=bad),
                 lambda: bare(ve.EpisodeMemory, _env=env, _lib=NoNativeCalls(), _h=1).Step(0, repeat=bad),
                 lambda: bare(ve.Actor, _env=env, _lib=NoNativeCalls(), _h=1, _out=0).Step(0.0, 0, 0, repeat=bad)):
        with pytest.raises(ValueError, match="repeat"):
            call()
    with pytest.raises(ValueError, match="repeat"):
        env.StepRepeatDevice(0, True)                             # a bool is not a count


# ---- pass without the feature: the model itself, on sequences worked by hand ---------------------------------------------------------
def test_model_cartpole_lane_that_terminates_at_substep_1_of_4(oracle):
    # lane 0: x just inside the track, moving out: one step stays inside, the second leaves (|x| > 2.4); lane 1: at rest, survives all four
    s0 = np.array([[2.39, 0.0], [0.4, 0.0], [0.0, 0.0], [0.0, 0.0]], F32)
    a = np.array([1, 0], np.int32)
    step1 = oracle.cartpole_step(s0, a, dtype=F32)
    step2 = oracle.cartpole_step(step1[0], a, dtype=F32)
    assert step1[2].tolist() == [0, 0] and step2[2].tolist() == [1, 0]                 # the hand-worked premise
    m = model.RepeatModel("CartPole", s0, seed=7, auto_reset=True, stats=True)
    d = m.decision(a, 4, tick0=10)
    assert d["finished_at"].tolist() == [1, -1] and d["done"].tolist() == [1, 0]
    assert d["reward"].tolist() == [2.0, 4.0]                                          # two steps taken, then idle; four steps
    assert d["fin_len"].tolist() == [2, 0] and d["fin_ret"].tolist() == [2.0, 0.0]
    assert d["ep_len"].tolist() == [0, 4] and d["ep_ret"].tolist() == [0.0, 4.0]       # env steps, not decisions
    # the finished lane sits on the reset draw of tick 10 + 1, untouched by sub-steps 2 and 3
    assert np.array_equal(d["state"][:, 0], oracle.cartpole_reset(7, 0, 11, 2)[:, 0])
    assert np.array_equal(d["final_obs"][:, 0], step2[0][:, 0])
    # without auto-reset the lane stays on its terminal state with steps_beyond_done as the one step left it
    m = model.RepeatModel("CartPole", s0, seed=7, auto_reset=False)
    d = m.decision(a, 4, tick0=10)
    assert np.array_equal(d["state"][:, 0], step2[0][:, 0]) and d["sbd"].tolist() == [0, -1] and m.after_done == 0
    d = m.decision(a, 4, tick0=14)                                                     # already done: ONE sub-step, reward 0, counted
    assert d["finished_at"].tolist() == [0, -1] and d["reward"].tolist() == [0.0, 4.0] and d["sbd"].tolist() == [1, -1] and m.after_done == 1


def test_model_mountaincar_lane_that_truncates_at_substep_0(oracle):
    s0 = np.array([[-0.5, -0.5], [0.0, 0.0]], F32)
    a = np.array([2, 0], np.int32)
    m = model.RepeatModel("MountainCar", s0, seed=3, auto_reset=True, stats=True, limit=5, len0=[4, 0])
    d = m.decision(a, 4, tick0=0)
    assert d["finished_at"].tolist() == [0, -1] and d["done"].tolist() == [2, 0]       # the time limit, at the first sub-step
    assert d["reward"].tolist() == [-1.0, -4.0] and d["fin_len"].tolist() == [5, 0] and d["ep_len"].tolist() == [0, 4]
    fresh, fresh_obs = model.reset_draw("MountainCar", 3, 0, 0, 2)
    assert np.array_equal(d["state"][:, 0], fresh[:, 0]) and np.array_equal(d["obs"][:, 0], fresh_obs[:, 0])
    one = oracle.env_step("MountainCar-v0", s0, a, dtype=F32)
    assert np.array_equal(d["final_obs"][:, 0], one[1][:, 0])
    d = m.decision(a, 4, tick0=4)                                                      # lane 1 reaches the limit at sub-step 0 of THIS decision
    assert d["finished_at"].tolist() == [-1, 0] and d["done"].tolist() == [0, 2] and d["fin_len"].tolist() == [5, 5]


def test_model_keeps_a_negative_zero_first_reward():
    # MountainCarContinuous: reward = (done ? 100 : 0) - a * a * 0.1; a = 0 gives 0 - 0 = +0.0 ... and a Pendulum-style -0.0 needs
    # -(0 + 0 + 0): restated here with the model's own accumulation rule on rewards given by hand
    rw = [np.array([-0.0, -0.0, 1.0], F32), np.array([-0.0, 2.0, -0.0], F32)]
    live = [np.array([True, True, True]), np.array([False, True, True])]
    reward = None
    for r in range(2):
        reward = rw[r].copy() if r == 0 else np.where(live[r], (reward + rw[r]).astype(F32), reward).astype(F32)
    assert np.signbit(reward[0]) and reward[0] == 0.0                                  # idle after sub-step 0: -0.0 survives
    assert reward.tolist() == [0.0, 2.0, 1.0] and not np.signbit(reward[2])
    assert not np.signbit((F32(0.0) + F32(-0.0)))                                      # what starting from 0.0f would have made of it
    # and through the model: a resting Pendulum at the top with zero torque earns -(0 + 0 + 0) = -0.0 on the first sub-step
    m = model.RepeatModel("Pendulum", np.zeros((2, 1), F32), seed=1, auto_reset=True, stats=True, limit=1)
    d = m.decision(np.zeros(1, F32), 4, tick0=0)
    assert d["finished_at"].tolist() == [0] and d["reward"][0] == 0.0 and np.signbit(d["reward"][0])
