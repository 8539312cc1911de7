"""CPU checks of the advantage / return feature (no GPU).  Fail without the feature: the library exports gymnet_gae_device and the
header, the ctypes mirror and Native.cs declare it with 14 parameters at ABI 6, the .hpp and VectorEnv.cs call it with that arity;
VectorEnv.AdvantagesDevice refuses every bad argument before any native call and hands good ones to gymnet_gae_device; build.py lists the
unit and its header.  Pass without it (they test the yardstick): the C twin against the float64 restatement over the GPU test's inputs,
and the twin's special cases, exact."""
import ctypes
import importlib
import os
import re
import sys

import numpy as np
import pytest

import _advantage_forms as forms
import _advantage_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAME, ARITY = "gymnet_gae_device", 14
# the twin's worst absolute deviation from the float64 restatement over every case below, measured on the CPU (see the test's docstring)
MEASURED_WORST = 4.68e-6


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


# ---- the yardstick --------------------------------------------------------------------------------------------------------------------
def test_twin_against_the_float64_restatement_over_the_gpu_tests_inputs():
    """Every (T, n) the GPU test runs at the small lane counts, and its wide lane counts at T = 9 and 33, gamma 0.99, lambda 0.95, with values, last value and boot (the form that exercises every term), and
    the lean form without values.  Measured worst |twin - float64| over advantage and return: 4.68e-6 (inputs are standard normal, so
    |A| reaches about 10 and one float32 spacing there is 9.5e-7: a few roundings of the carried sum); asserted at 4 x that, the margin
    being for other seeds.  The value is the twin's against the float64 reference, not the kernel's: the kernel is held to the twin's bits."""
    worst = 0.0
    steps = twin.steps_for(forms.U.values())
    for T, n in [(T, n) for T in steps for n in twin.NS] + [(T, n) for T in (twin.WIDE_T, steps[-1]) for n in twin.WIDE_NS]:
        c = twin.case(T, n)
        for v, vlast, boot in ((c["v"][:T], c["v"][T], c["boot"]), (None, None, None)):
            adv, ret = twin.gae(c["r"], c["d"], v, vlast, boot)
            adv64, ret64 = twin.gae64(c["r"], c["d"], v, vlast, boot)
            worst = max(worst, float(np.abs(adv - adv64).max()), float(np.abs(ret - ret64).max()))
    print(f"worst |twin - float64| = {worst:.3e} (asserted at {4 * MEASURED_WORST:.3e})")
    assert worst <= 4 * MEASURED_WORST


def test_lambda_zero_is_the_one_step_td_error_and_gamma_zero_is_r_minus_v():
    c = twin.case(9, 252, seed=1)
    r, d, v, vlast, boot = c["r"], c["d"], c["v"][:9], c["v"][9], c["boot"]
    vnext = np.concatenate([v[1:], vlast[None]])
    for b in (boot, None):
        nv = np.where(d & 1, F32(0), np.where(d & 2, F32(0) if b is None else b, vnext)).astype(F32)
        # fmaf(gamma, nv, r) in float64: the product of two float32 is exact there and the sum is within 2^-29 of a float32 spacing of exact
        want = ((np.float64(F32(0.99)) * nv.astype(np.float64) + r.astype(np.float64)).astype(F32) - v).astype(F32)
        adv, ret = twin.gae(r, d, v, vlast, b, gamma=0.99, lam=0.0)
        assert twin.same(adv, want) and twin.same(ret, (want + v).astype(F32))
        adv, ret = twin.gae(r, d, v, vlast, b, gamma=0.0, lam=0.95)
        assert twin.same(adv, (r - v).astype(F32)) and twin.same(ret, ((r - v).astype(F32) + v).astype(F32))


def test_no_values_at_gamma_and_lambda_one_is_the_integer_return_to_go():
    T, n = 33, 17
    rng = np.random.default_rng(3)
    d = (rng.random((T, n)) < 0.15).astype(np.uint8) * rng.integers(1, 4, (T, n)).astype(np.uint8)
    r = np.ones((T, n), F32)                                       # CartPole's reward
    adv, ret = twin.gae(r, d, None, None, None, gamma=1.0, lam=1.0)
    want = np.zeros((T, n), F32)
    for i in range(n):
        run = 0
        for t in range(T - 1, -1, -1):
            run = 1 if d[t, i] else run + 1
            want[t, i] = run
    assert twin.same(adv, want) and twin.same(ret, want)


def _one_lane(r, d, v, vlast, boot, gamma, lam):
    col = lambda x: None if x is None else np.asarray(x, F32).reshape(-1, 1)
    adv, ret = twin.gae(col(r), np.asarray(d, np.uint8).reshape(-1, 1), col(v), None if vlast is None else np.asarray([vlast], F32), col(boot), gamma, lam)
    return adv[:, 0].tolist(), ret[:, 0].tolist()


def test_done_bytes_with_and_without_boot_hand_worked():
    """gamma = lambda = 0.5 (gl = 0.25) and small dyadic numbers: every product and sum below is exact in float32"""
    r, v, boot, vlast = [1.0, 2.0, 4.0], [0.5, 0.25, 1.0], [8.0, 16.0, 32.0], 2.0
    # no done: delta2 = 4 + .5*2 - 1 = 4; delta1 = 2 + .5*1 - .25 = 2.25; delta0 = 1 + .5*.25 - .5 = .625
    adv, ret = _one_lane(r, [0, 0, 0], v, vlast, boot, 0.5, 0.5)
    assert adv == [0.625 + 0.25 * (2.25 + 0.25 * 4.0), 2.25 + 0.25 * 4.0, 4.0] and ret == [adv[0] + 0.5, adv[1] + 0.25, adv[2] + 1.0]
    for byte, with_boot, nv in ((1, True, 0.0), (1, False, 0.0), (2, True, 16.0), (2, False, 0.0), (3, True, 0.0), (3, False, 0.0)):
        # a done on row 1: row 1 bootstraps from nv (terminated wins over truncated), and row 0 restarts its sum at row 1's cut
        adv, _ = _one_lane(r, [0, byte, 0], v, vlast, boot if with_boot else None, 0.5, 0.5)
        d1 = 2.0 + 0.5 * nv - 0.25
        assert adv == [0.625 + 0.25 * d1, d1, 4.0], (byte, with_boot, adv)
        # a done on the last row: the last value is not used; on row 0: nothing upstream of it exists, row 1 is unaffected
        adv, _ = _one_lane(r, [0, 0, byte], v, vlast, boot if with_boot else None, 0.5, 0.5)
        nv2 = 32.0 if (byte == 2 and with_boot) else 0.0
        d2 = 4.0 + 0.5 * nv2 - 1.0
        assert adv == [0.625 + 0.25 * (2.25 + 0.25 * d2), 2.25 + 0.25 * d2, d2], (byte, with_boot, adv)
        adv, _ = _one_lane(r, [byte, 0, 0], v, vlast, boot if with_boot else None, 0.5, 0.5)
        nv0 = 8.0 if (byte == 2 and with_boot) else 0.0
        assert adv == [1.0 + 0.5 * nv0 - 0.5, 2.25 + 0.25 * 4.0, 4.0], (byte, with_boot, adv)
    # consecutive dones: every row is its own segment
    adv, _ = _one_lane(r, [1, 2, 3], v, vlast, boot, 0.5, 0.5)
    assert adv == [0.5, 2.0 + 8.0 - 0.25, 3.0]
    # without values the last value and boot still count
    adv, ret = _one_lane(r, [0, 2, 0], None, vlast, boot, 0.5, 0.5)
    assert adv == [1.0 + 0.25 * 10.0, 2.0 + 8.0, 4.0 + 1.0] and ret == adv


# ---- fail without the feature -------------------------------------------------------------------------------------------------------
def test_the_call_is_exported_and_declared_with_fourteen_parameters(gymnet):
    capi = importlib.import_module(gymnet.__name__ + "._capi")
    lib = ctypes.CDLL(gymnet.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gymnet_amd.h")).read(), flags=re.S)
    native = re.sub(r"//.*", "", open(os.path.join(ROOT, "gym.net_amd", "csharp", "Native.cs")).read())
    hpp = open(os.path.join(ROOT, "include", "gymnet_amd.hpp")).read()
    vcs = open(os.path.join(ROOT, "gym.net_amd", "csharp", "VectorEnv.cs")).read()
    assert hasattr(lib, NAME)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m and len(_split_args(m.group(1))) == ARITY
    assert len(capi.PROTOTYPES[NAME][1]) == ARITY
    cs = re.search(r"\[DllImport\(Lib\)\] public static extern int %s\(([^;]*)\);" % NAME, native)
    assert cs and len(_split_args(cs.group(1))) == ARITY
    call = re.search(NAME + r"\(([^;]*)\)\);", hpp)
    assert call and len(_split_args(call.group(1))) == ARITY
    call = re.search(r"Native\." + NAME + r"\(([^;]*)\)\);", vcs)
    assert call and len(_split_args(call.group(1))) == ARITY
    assert capi.ABI_VERSION == 6 and re.search(r"#define\s+GYMNET_ABI_VERSION\s+6\b", hdr)
    assert "AdvantagesDevice(" in hpp and "AdvantagesDevice(" in vcs
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")
    assert callable(ve.VectorEnv.AdvantagesDevice)


def test_the_unit_is_a_build_input():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    assert "advantage.hip" in kernel_resources._BUILD.SOURCES and "advantage.hip" in kernel_resources._BUILD.DEPS
    assert "advantage.hpp" in kernel_resources._BUILD.DEPS
    assert "advantage" not in kernel_resources.ENVS and "advantage" not in kernel_resources.CLI_ENVS    # collect()'s default is untouched


class _Tensor:
    """what the argument checks look at, without a GPU"""

    def __init__(self, shape, dtype="torch.float32", cuda=True, contiguous=True, ptr=4096):
        self.shape, self.dtype, self.is_cuda, self._contiguous, self._ptr = tuple(shape), dtype, cuda, contiguous, ptr

    def data_ptr(self):
        return self._ptr

    def is_contiguous(self):
        return self._contiguous


class OnlyTheView:
    """the library as the checks may use it: nothing but the handle's device view (where the stream comes from), after every check"""

    def gymnet_vecenv_device_view(self, h, view):
        return 0

    def __getattr__(self, name):
        raise AssertionError("native call: " + name)


def test_advantage_arguments_are_checked_before_any_native_call(gymnet):
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")
    N, T = 12, 5
    env = ve.VectorEnv.__new__(ve.VectorEnv)
    env.__dict__.update(_lib=OnlyTheView(), _h=1, _owns_handle=False, NumberOfEnvironments=N, Device=0)
    f = lambda *shape, **kw: _Tensor(shape, **kw)
    u8 = lambda *shape, **kw: _Tensor(shape, dtype="torch.uint8", **kw)
    good = dict(reward=f(T, N), done=u8(T, N), values=f(T, N), advantage=f(T, N), returns=f(T, N), last_value=f(N), boot=f(T, N))
    bad = {
        "reward": (f(T, N, dtype="torch.float64"), f(T, N + 1), f(T * N), f(T, N, cuda=False), f(T, N, contiguous=False), np.zeros((T, N), F32), 4096, None),
        "done": (f(T, N), _Tensor((T, N), "torch.bool"), _Tensor((T, N), "torch.int32"), u8(T + 1, N), u8(T, N + 1), u8(T, N, cuda=False),
                 u8(T, N, contiguous=False), np.zeros((T, N), np.uint8), None),
        "values": (f(T, N, dtype="torch.float16"), f(T - 1, N), f(T + 2, N), f(T, N + 1), f(T, N, cuda=False), f(T, N, contiguous=False), f(T + 1, N),
                   np.zeros((T, N), F32)),                       # (T + 1 rows beside a last_value)
        "last_value": (f(N, dtype="torch.float64"), f(N + 1), f(1, N), f(N, cuda=False), f(N, contiguous=False), 0.0),
        "boot": (f(T, N, dtype="torch.float64"), f(T + 1, N), f(T, N + 1), f(T, N, cuda=False), f(T, N, contiguous=False), np.zeros((T, N), F32)),
        "advantage": (f(T, N, dtype="torch.float64"), f(T + 1, N), f(N, T), f(T, N, cuda=False), f(T, N, contiguous=False), 4096),
        "returns": (f(T, N, dtype="torch.float64"), f(T + 1, N), f(N, T), f(T, N, cuda=False), f(T, N, contiguous=False), 4096),
        "gamma": (-0.1, 1.5, float("nan"), float("inf"), None, "0.9", True),
        "lam": (-0.1, 1.5, float("nan"), None, True),
    }
    for name, values in bad.items():
        for value in values:
            with pytest.raises(ValueError):
                env.AdvantagesDevice(**dict(good, **{name: value}))
    with pytest.raises(ValueError):
        env.AdvantagesDevice(**dict(good, advantage=None, returns=None))
    with pytest.raises(ValueError):                                # T disagreeing between arguments
        env.AdvantagesDevice(**dict(good, reward=f(T + 1, N)))
    reach = "native call: " + NAME
    with pytest.raises(AssertionError, match=reach):               # good arguments do reach the library
        env.AdvantagesDevice(**good)
    for change in (dict(values=None), dict(values=None, last_value=None, boot=None), dict(values=f(T + 1, N), last_value=None), dict(advantage=None),
                   dict(returns=None), dict(last_value=None), dict(boot=None)):
        with pytest.raises(AssertionError, match=reach):
            env.AdvantagesDevice(**dict(good, **change))
    import inspect
    sig = inspect.signature(ve.VectorEnv.AdvantagesDevice)
    assert list(sig.parameters)[1:] == ["reward", "done", "values", "advantage", "returns", "gamma", "lam", "last_value", "boot"]
    assert (sig.parameters["gamma"].default, sig.parameters["lam"].default) == (0.99, 0.95)
    assert "AdvantagesDevice" not in getattr(gymnet, "__all__", ())   # nothing new exported beyond what VectorEnv carries
