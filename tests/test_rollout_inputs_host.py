"""CPU checks of the rollout-inputs feature (no GPU).  Pass without the feature (they test the yardstick): the NumPy twin
(tests/_rollout_inputs_twin.py) against the history model the attachment tests use for Push, against a second formulation that looks
back over the done bytes instead of pushing, and on hand-worked cases; the float64 rounding cases are what they claim to be.  Fail without
it: the library exports both calls and every layer declares them with the header's arity at ABI 6; the library refuses every bad call
before it touches a device and writes the reason; VectorEnv.RolloutInputsDevice and Actor.HistoryDevice check their arguments before any
native call; build.py lists the unit and its header; the compiled kernel set is the table of tests/_rollout_inputs_forms.py, with no
scratch and no LDS."""
import ctypes
import importlib
import os
import re
import sys

import numpy as np
import pytest

import _actor_twin as atwin
import _rollout_inputs_forms as forms
import _rollout_inputs_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, U32 = np.float32, np.uint32
EXPORTS = {"gymnet_rollout_inputs_device": 18, "gymnet_vecenv_actor_history_device": 3}


# ---- the yardstick --------------------------------------------------------------------------------------------------------------------
def looking_back(rec_obs, rec_done, history0):
    """the second formulation: slot s of the input of step t is observation max(t - S + s, last), where observation j >= 0 is
    rec_obs[j], j < 0 is history0[S + j], and last is the newest row below t whose done byte is set"""
    obs, h0 = twin.f32_bits(rec_obs), twin.f32_bits(history0)
    S, O, n = h0.shape
    T = obs.shape[0]
    x = np.empty((T + 1, n, S, O), U32)
    for i in range(n):
        for t in range(T + 1):
            last = max([r for r in range(t) if rec_done[r, i] != 0], default=-10 ** 9)
            for s in range(S):
                j = max(t - S + s, last)
                x[t, i, s] = obs[j, :, i] if j >= 0 else h0[S + j, :, i]
    return x[:T].reshape(T, n, S * O), np.ascontiguousarray(x[T].transpose(1, 2, 0))


@pytest.mark.parametrize("O,S", [(4, 4), (4, 1), (3, 5), (1, 9)])
def test_twin_agrees_with_the_attachment_tests_history_model_and_with_looking_back(O, S):
    n = 5
    for T in twin.steps_for(S)[:-1] + (19,):
        for pattern in twin.PATTERNS:
            c = twin.case(O, S, T, n, pattern, seed=11)
            model = atwin.History(np.zeros((n, O), F32), S)
            model.h = np.ascontiguousarray(c["history0"].transpose(2, 0, 1)).copy()           # [n, S, O]: the history the rollout starts from
            for t in range(T):
                assert np.array_equal(model.x().view(U32), c["x"][t]), (T, pattern, t)
                model.push(c["rec_obs"][t].T, c["rec_done"][t])
            assert np.array_equal(model.h.view(U32), c["history_out"].transpose(2, 0, 1)), (T, pattern)
            x, h = looking_back(c["rec_obs"], c["rec_done"], c["history0"])
            assert np.array_equal(x, c["x"]) and np.array_equal(h, c["history_out"]), (T, pattern)
    c = twin.case(O, S, 7, 3, "bernoulli", seed=12, f64=True)
    x, h = looking_back(c["rec_obs"], c["rec_done"], c["history0"])
    assert np.array_equal(x, c["x"]) and np.array_equal(h, c["history_out"])


def test_hand_worked_rows():
    """one lane, obs_dim 1, S = 3, history0 = (-3, -2, -1), observations 10, 11, 12, 13, 14 with a done on rows 1 and 2"""
    obs = np.array([10, 11, 12, 13, 14], F32).reshape(5, 1, 1)
    done = np.array([0, 1, 2, 0, 0], np.uint8).reshape(5, 1)
    h0 = np.array([-3, -2, -1], F32).reshape(3, 1, 1)
    x, h = twin.inputs(obs, done, h0)
    assert x.view(F32).reshape(5, 3).tolist() == [[-3, -2, -1], [-2, -1, 10], [11, 11, 11], [12, 12, 12], [12, 12, 13]]
    assert h.view(F32).reshape(3).tolist() == [12, 13, 14]
    assert twin.gathered(x, [4, 0, 0, 5, -1]).view(U32).tolist() == [x[4, 0].tolist(), x[0, 0].tolist(), x[0, 0].tolist(), [twin.NAN_BITS] * 3, [twin.NAN_BITS] * 3]
    x0, h00 = twin.inputs(obs[:0], done[:0], h0)                           # no steps: only the history
    assert x0.shape == (0, 1, 3) and np.array_equal(h00, h0.view(U32))
    # a rollout cut in two chains through the history
    xa, ha = twin.inputs(obs[:2], done[:2], h0)
    xb, hb = twin.inputs(obs[2:], done[2:], ha.view(F32))
    assert np.array_equal(np.concatenate([xa, xb]), x) and np.array_equal(hb, h)


def test_the_inputs_carry_the_values_they_claim():
    bits = twin.random_bits((4, 4, 5), np.random.default_rng(0)).view(U32).reshape(-1)
    assert tuple(bits[:len(twin.SPECIAL_BITS)]) == twin.SPECIAL_BITS
    v = np.array(twin.SPECIAL_BITS, U32).view(F32)
    assert np.signbit(v[0]) and v[0] == 0 and 0 < v[2] < np.finfo(F32).tiny and np.isinf(v[4:6]).all() and np.isnan(v[6:]).all()
    got = twin.f32_bits(np.array(twin.F64_SPECIALS, np.float64)).view(F32)
    one_up = np.nextafter(F32(1), F32(2))
    assert got[0] == 1.0 and got[1] == np.nextafter(one_up, F32(2)) and got[2] == -1.0 and got[3] == one_up and got[4] == 1.0          # ties to even, and off a tie
    assert np.isinf(got[5]) and got[6] == np.finfo(F32).max and got[7] == np.inf and got[8] == -np.inf and got[9] == np.inf
    assert (got[10:14] == 0).all() and np.signbit(got[11]) and not np.signbit(got[10])
    den = got[14:21].view(U32)
    assert den[2] == 1 and den[3] == 0 and den[4] == 2 and den[5] == 1 and den[6] == 0x00800000                      # 2^-150 ties to 0, 3 x 2^-150 to 2 x 2^-149
    assert 0 < got[14] < np.finfo(F32).tiny and got[15] == -got[14]
    for pattern in twin.PATTERNS:
        d = twin.done_pattern(pattern, 37, 67, 4, np.random.default_rng(1))
        assert d.dtype == np.uint8 and d.max() <= 3 and (d.any() == (pattern != "none"))
    d = twin.done_pattern("both_bits", 37, 67, 4, np.random.default_rng(1))
    assert set(np.unique(d)) == {0, 1, 2, 3}
    d = twin.done_pattern("runs", 37, 67, 4, np.random.default_rng(1))
    assert ((d[1:] != 0) & (d[:-1] != 0)).any()


# ---- fail without the feature -------------------------------------------------------------------------------------------------------
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


def test_both_calls_are_exported_and_declared_in_every_layer(gymnet):
    capi = importlib.import_module(gymnet.__name__ + "._capi")
    lib = ctypes.CDLL(gymnet.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gymnet_amd.h")).read(), flags=re.S)
    native = re.sub(r"//.*", "", open(os.path.join(ROOT, "gym.net_amd", "csharp", "Native.cs")).read())
    hpp = open(os.path.join(ROOT, "include", "gymnet_amd.hpp")).read()
    vcs = open(os.path.join(ROOT, "gym.net_amd", "csharp", "VectorEnv.cs")).read()
    for name, arity in EXPORTS.items():
        assert hasattr(lib, name)
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m and len(_split_args(m.group(1))) == arity, name
        assert len(capi.PROTOTYPES[name][1]) == arity
        cs = re.search(r"\[DllImport\(Lib\)\] public static extern int %s\(([^;]*)\);" % name, native)
        assert cs and len(_split_args(cs.group(1))) == arity, name
        call = re.search(name + r"\(([^;]*)\)\);", hpp)
        assert call and len(_split_args(call.group(1))) == arity, name
        call = re.search(r"Native\." + name + r"\(([^;]*)\)\);", vcs)
        assert call and len(_split_args(call.group(1))) == arity, name
    assert capi.ABI_VERSION == 6 and re.search(r"#define\s+GYMNET_ABI_VERSION\s+6\b", hdr)
    for wrapper in ("ActorHistoryDevice(", "RolloutInputsDevice("):
        assert wrapper in hpp and wrapper in vcs
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")
    assert callable(ve.VectorEnv.RolloutInputsDevice) and callable(ve.Actor.HistoryDevice)


def test_the_unit_is_a_build_input():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    assert "rollout_inputs.hip" in kernel_resources._BUILD.SOURCES and "rollout_inputs.hip" in kernel_resources._BUILD.DEPS
    assert "rollout_inputs.hpp" in kernel_resources._BUILD.DEPS


def test_the_mirror_restates_the_header_and_the_unit():
    hpp = open(os.path.join(ROOT, "gym.net_amd", "csrc", "rollout_inputs.hpp")).read()
    src = open(os.path.join(ROOT, "gym.net_amd", "csrc", "rollout_inputs.hip")).read()
    assert re.search(r"constexpr int64_t kRolloutInputsMinRows = (\d+);", hpp).group(1) == str(forms.MIN_ROWS)
    assert eval(re.search(r"constexpr int64_t kRolloutInputsTargetThreads = ([0-9 *]+);", hpp).group(1)) == forms.TARGET_THREADS
    assert re.search(r"constexpr int kRolloutInputsBlock = (\d+);", hpp).group(1) == str(forms.BLOCK)
    assert re.search(r"constexpr int kRowsInFlight = (\d+);", src).group(1) == str(forms.ROWS_IN_FLIGHT)
    assert forms.vec_for(16, 16, 4096) == 4 and forms.vec_for(16, 19, 4096) == 1 and forms.vec_for(16, 16, 4100) == 1 and forms.vec_for(63, 64, 4096) == 1
    assert forms.chunks_for(37, 1028, 4, 4, 4) == (8, 5) and forms.chunks_for(256, 1 << 16, 4, 4, 4) == (32, 8)      # tests/cpp/rollout_inputs_test.cpp
    assert forms.chunks_for(100, 1028, 2, 32, 4) == (32, 4) and forms.chunks_for(16, 1 << 20, 4, 4, 4) == (16, 1)


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    return kernel_resources.collect(("rollout_inputs.hip",))


@pytest.mark.timeout(900)
def test_forms_table_names_every_compiled_kernel_and_none_uses_scratch_or_lds(kernels):
    table = sorted([row["kernel"] for row in forms.FORMS] + forms.HISTORY_KERNELS)
    assert len(table) == len(set(table)) == 10
    assert sorted(kernels) == table, (sorted(set(kernels) - set(table)), sorted(set(table) - set(kernels)))
    for row in forms.FORMS:
        r = row["reach"]
        width = r["obs_dim"] * r["history"]
        assert forms.row_kernel(forms.vec_for(width, width + r["pad"], 4 * r["offset"]), row["f64"], row["gathered"]) == row["kernel"]
    for name in sorted(kernels):
        k = kernels[name]
        print(f"{name:48s} VGPRs {k['vgpr']:3d}  waves {k['occupancy']}  scratch {k['scratch']}  LDS {k['lds']}")
        assert k["scratch"] == 0 and k["lds"] == 0 and k["occupancy"] >= 4, (name, k)


def test_the_library_refuses_bad_calls_before_it_touches_a_device(gymnet):
    """through the C ABI with made-up addresses: every refusal returns before any HIP call, so this runs without a GPU"""
    capi = importlib.import_module(gymnet.__name__ + "._capi")
    lib = capi.load_library()
    good = dict(steps=5, count=12, stride=12, obs_dim=4, history=4, f64=0, obs=0x10000, done=0x20000, h0=0x30000, h0s=12, rows=None, m=0, x=0x40000, xrs=16,
                hout=0x50000, hs=12)

    def call(**change):
        a = dict(good, **change)
        p = lambda v: None if v is None else ctypes.c_void_p(v)
        return lib.gymnet_rollout_inputs_device(0, None, a["steps"], a["count"], a["stride"], a["obs_dim"], a["history"], a["f64"], p(a["obs"]), p(a["done"]),
                                                p(a["h0"]), a["h0s"], p(a["rows"]), a["m"], p(a["x"]), a["xrs"], p(a["hout"]), a["hs"])
    refused = {"negative": [dict(steps=-1), dict(count=-1), dict(stride=-1), dict(h0s=-1), dict(xrs=-1), dict(hs=-1), dict(rows=0x60000, m=-1)],
               ">= 1": [dict(obs_dim=0), dict(history=0)], "beyond 64": [dict(history=17)],
               "stride < count": [dict(stride=11)], "history0_stride < count": [dict(h0s=11)], "history_out_stride < count": [dict(hs=11)],
               "x_row_stride <": [dict(xrs=15)], "null with steps > 0": [dict(obs=None), dict(done=None), dict(h0=None)],
               "needs d_history0": [dict(steps=0, h0=None)], "d_x is null": [dict(x=None), dict(x=None, rows=0x60000, m=2)],
               "aligned": [dict(obs=0x10002), dict(f64=1, obs=0x10004), dict(h0=0x30001), dict(x=0x40002), dict(hout=0x50003), dict(rows=0x60004, m=2)],
               "alias": [dict(x=0x10000), dict(x=0x20000), dict(x=0x30000), dict(hout=0x30000), dict(rows=0x60000, m=2, x=0x60000)],
               "same array": [dict(hout=0x40000)], "overflow": [dict(steps=2 ** 61)]}
    for word, changes in refused.items():
        for change in changes:
            assert call(**change) == capi.ERR_INVALID_ARG, change
            msg = lib.gymnet_last_error().decode()
            assert msg.startswith("rollout_inputs: ") and word in msg, (change, msg)
    # what needs no launch succeeds without a device: no steps and no history asked for, no lanes, a gathered form with no row
    assert call(steps=0, hout=None) == 0 and call(count=0, stride=0) == 0 and call(rows=0x60000, m=0) == 0
    assert lib.gymnet_vecenv_actor_history_device(None, None, 0) == capi.ERR_INVALID_ARG


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


def test_arguments_are_checked_before_any_native_call(gymnet):
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")
    N, T, O, S = 12, 5, 4, 4
    env = ve.VectorEnv.__new__(ve.VectorEnv)
    env.__dict__.update(_lib=OnlyTheView(), _h=1, _owns_handle=False, NumberOfEnvironments=N, Device=0, ObsDim=O)
    f = lambda *shape, **kw: _Tensor(shape, **kw)
    good = dict(rec_obs=f(T, O, N), rec_done=f(T, N, dtype="torch.uint8"), history0=f(S, O, N), history=S, rows=None, out=f(T, N, S * O), history_out=f(S, O, N))
    bad = {
        "rec_obs": (f(T, O, N, dtype="torch.float16"), f(T, O, N + 1), f(T, O * N), f(T, O, N, cuda=False), f(T, O, N, contiguous=False), np.zeros((T, O, N), F32), None),
        "rec_done": (f(T, N), f(T, N, dtype="torch.bool"), f(T + 1, N, dtype="torch.uint8"), f(T, N, dtype="torch.uint8", cuda=False),
                     f(T, N, dtype="torch.uint8", contiguous=False), None),
        "history0": (f(S, O, N, dtype="torch.float64"), f(S + 1, O, N), f(S, O, N + 1), f(N, S, O), f(S, O, N, cuda=False), f(S, O, N, contiguous=False), None),
        "history": (0, -1, 65, 17, 4.0, True, None),
        "rows": (f(7, dtype="torch.int32"), f(7, 1, dtype="torch.int64"), f(7, dtype="torch.int64", cuda=False), f(7, dtype="torch.int64", contiguous=False), [0, 1]),
        "out": (f(T, N, S * O, dtype="torch.float64"), f(T * N, S * O), f(T, N, S * O + 3), f(T, N, S * O, cuda=False), f(T, N, S * O, contiguous=False)),
        "history_out": (f(S, O, N, dtype="torch.float64"), f(S, O, N + 5), f(S, O, N, cuda=False), f(S, O, N, contiguous=False)),
    }
    for name, values in bad.items():
        for value in values:
            with pytest.raises(ValueError):
                env.RolloutInputsDevice(**dict(good, **{name: value}))
    reach = "native call: gymnet_rollout_inputs_device"
    with pytest.raises(AssertionError, match=reach):               # good arguments do reach the library
        env.RolloutInputsDevice(**good)
    for change in (dict(history_out=None), dict(rec_obs=f(T, O, N, dtype="torch.float64")), dict(rows=f(7, dtype="torch.int64"), out=f(7, S * O)),
                   dict(history=1, history0=f(1, O, N), out=f(T, N, O), history_out=None)):
        with pytest.raises(AssertionError, match=reach):
            env.RolloutInputsDevice(**dict(good, **change))
    with pytest.raises(ValueError):                                # the gathered form's out is [m, width]
        env.RolloutInputsDevice(**dict(good, rows=f(7, dtype="torch.int64")))
    empty = f(0, S * O)
    assert env.RolloutInputsDevice(**dict(good, rows=f(0, dtype="torch.int64", ptr=0), out=empty)) is empty          # no row: no native call
    import inspect
    sig = inspect.signature(ve.VectorEnv.RolloutInputsDevice)
    assert list(sig.parameters)[1:] == ["rec_obs", "rec_done", "history0", "history", "rows", "out", "history_out"]
    # Actor.HistoryDevice: a caller's tensor is [history, obs_dim, N] float32 on the device
    actor = ve.Actor.__new__(ve.Actor)
    actor.__dict__.update(_env=env, _lib=env._lib, _h=1, History_=S)
    for value in (f(S, O, N, dtype="torch.float64"), f(N, S, O), f(S, O, N + 1), f(S, O, N, cuda=False), f(S, O, N, contiguous=False), np.zeros((S, O, N), F32)):
        with pytest.raises(ValueError):
            actor.HistoryDevice(value)
    with pytest.raises(AssertionError, match="native call: gymnet_vecenv_actor_history_device"):
        actor.HistoryDevice(f(S, O, N))
