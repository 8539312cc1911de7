"""CPU checks of gymnet_vecenv_actor_policy_gradient / _value_gradient: exported, one arity in every binding, additive in ABI 6, refused on
a null handle, built from csrc/actor_grad.hip / .hpp.  Every test fails without the feature: the exports do not exist."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

ROOT =os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_read = lambda *parts: open(os.path.join(ROOT, *parts)).read()            # noqa: E731
CALLS = {"gymnet_vecenv_actor_policy_gradient": ("ActorPolicyGradient", 14), "gymnet_vecenv_actor_value_gradient": ("ActorValueGradient", 10)}


def _arity(text, pattern):
    """parameters of the first declaration or call that `pattern` opens (its match ends at the opening parenthesis)"""
    m = re.search(pattern, text)
    assert m, pattern
    depth, start = 0, m.end() - 1
    for i in range(start, len(text)):
        depth += (text[i] == "(") - (text[i] == ")")
        if depth == 0:
            return len([a for a in text[start + 1:i].split(",") if a.strip()])
    raise AssertionError("unbalanced")


@pytest.mark.parametrize("export", CALLS)
def test_one_arity_in_every_binding(gymnet, export):
    method, arity = CALLS[export]
    assert hasattr(ctypes.CDLL(gymnet.LIB_PATH), export)
    header = re.sub(r"/\*.*?\*/", " ", _read("include", "gymnet_amd.h"), flags=re.S)
    assert _arity(header, r"\bint\s+" + export + r"\s*\(") == arity
    assert len(gymnet._capi.PROTOTYPES[export][1]) == arity
    assert _arity(_read("gym.net_amd", "csharp", "Native.cs"), r"extern int " + export + r"\(") == arity
    assert _arity(_read("include", "gymnet_amd.hpp"), r"check\(" + export + r"\(") == arity
    assert _arity(_read("gym.net_amd", "csharp", "VectorEnv.cs"), r"Native\." + export + r"\(") == arity
    assert ("void " + method + "(") in _read("include", "gymnet_amd.hpp") and ("public void " + method + "(") in _read("gym.net_amd", "csharp", "VectorEnv.cs")
    assert callable(getattr(importlib.import_module(gymnet.__name__ + ".vector_env").Actor, method[len("Actor"):]))


class _Tensor:
    """what the argument checks look at, without a GPU (x is also asked for dim() and stride())"""

    def __init__(self, shape, dtype="torch.float32", cuda=True, contiguous=True, strides=None):
        self.shape, self.dtype, self.is_cuda, self._contiguous = tuple(shape), dtype, cuda, contiguous
        self._strides = tuple(strides) if strides is not None else tuple(int(np.prod(shape[k + 1:])) for k in range(len(shape)))

    def data_ptr(self):
        return 4096

    def is_contiguous(self):
        return self._contiguous

    def dim(self):
        return len(self.shape)

    def stride(self, k=None):
        return self._strides if k is None else self._strides[k]


class NoNativeCalls:
    def __getattr__(self, name):
        raise AssertionError("native call: " + name)


def test_gradient_arguments_are_checked_before_any_native_call(gymnet):
    """every refusal of PolicyGradient and ValueGradient that needs no device: the kind, the critic, the flat weights, x with its own stride
    rule, the per-row tensors and grad.  (What follows them allocates on the device.)"""
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")
    N, m, W, count, ccount = 12, 7, 8, 90, 40
    env = ve.VectorEnv.__new__(ve.VectorEnv)
    env.__dict__.update(_lib=NoNativeCalls(), _h=1, _owns_handle=False, NumberOfEnvironments=N, Device=0)

    def actor(box, critic=(W, 4, 1)):
        o = ve.Actor.__new__(ve.Actor)
        o.__dict__.update(IsBox=box, _lib=env._lib, _h=1, _env=env, Widths=(W, 9, 2), Count=count, CriticWidths=critic, CriticCount=ccount)
        return o

    f = lambda *shape, **kw: _Tensor(shape, **kw)
    i32 = lambda *shape, **kw: _Tensor(shape, dtype="torch.int32", **kw)
    with pytest.raises(ValueError, match="Discrete"):
        actor(True).PolicyGradient(f(count), f(m, W), i32(m), f(m), grad=f(count))
    with pytest.raises(ValueError, match="critic"):
        actor(False, critic=None).ValueGradient(f(ccount), f(m, W), f(m), grad=f(ccount))
    a = actor(False)
    good = dict(net=f(count), x=f(m, W), actions=i32(m), coef=f(m), logp_old=f(m), logp=f(m), grad=f(count))
    rows = (f(m, dtype="torch.float64"), f(m + 1), f(m, 1), f(m, cuda=False), f(m, contiguous=False), np.zeros(m, np.float32), 4096)
    bad = {
        "net": (f(count + 1), f(count, dtype="torch.float64"), f(count, cuda=False), f(count, contiguous=False), np.zeros(count, np.float32), 4096, None),
        "x": (f(m, W + 1), f(m, W, dtype="torch.float64"), f(m, W, cuda=False), f(m), f(0, W), f(m, W, strides=(W, 2)), f(m, W, strides=(W - 1, 1)),
              np.zeros((m, W), np.float32), 4096, None),
        "actions": rows + (f(m),), "coef": rows + (i32(m),), "logp_old": rows, "logp": rows,
        "grad": (f(count + 1), f(count, dtype="torch.float64"), f(count, cuda=False), f(count, contiguous=False), 4096),
    }
    for name, values in bad.items():
        for value in values:
            with pytest.raises(ValueError, match=r"\b%s\b" % name):
                a.PolicyGradient(**dict(good, **{name: value}))
    vgood = dict(net=f(ccount), x=f(m, W), target=f(m), value=f(m), grad=f(ccount))
    for name, values in {"net": (f(count),), "x": (f(m, W + 1), f(m, W, strides=(W, 2))), "target": rows, "value": rows, "grad": (f(count),)}.items():
        for value in values:
            with pytest.raises(ValueError, match=r"\b%s\b" % name):
                a.ValueGradient(**dict(vgood, **{name: value}))
    with pytest.raises(ValueError, match="coef"):                  # rows at a stride beyond the width pass x's rule: the refusal is another argument's
        a.PolicyGradient(**dict(good, x=f(m, W, strides=(W + 5, 1)), coef=f(m + 1)))


def test_additive_in_abi_6_a_null_handle_is_refused_and_the_unit_is_a_build_input(gymnet):
    capi, build = gymnet._capi, importlib.import_module(gymnet.__name__ + ".build")
    lib = capi.load_library()
    assert capi.ABI_VERSION == 6 == lib.gymnet_abi_version()
    assert "actor_grad.hip" in build.SOURCES and "actor_grad.hip" in build.DEPS and "actor_grad.hpp" in build.DEPS
    assert lib.gymnet_vecenv_actor_policy_gradient(None, None, 0, None, 0, 0, None, None, None, 0.2, 0.0, None, None, None) == capi.ERR_INVALID_ARG
    assert lib.gymnet_vecenv_actor_value_gradient(None, None, 0, None, 0, 0, None, None, None, None) == capi.ERR_INVALID_ARG

