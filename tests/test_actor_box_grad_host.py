"""CPU checks of gymnet_vecenv_actor_box_policy_gradient, in the manner of test_actor_grad_host.py: exported, one arity in every binding,
additive in ABI 6, refused on a null handle.  Both tests fail without the feature: the export does not exist."""
import ctypes
import importlib

from test_actor_grad_host import _arity, _read

EXPORT, METHOD, ARITY = "gymnet_vecenv_actor_box_policy_gradient", "ActorBoxPolicyGradient", 15


def test_one_arity_in_every_binding(gymnet):
    import re
    assert hasattr(ctypes.CDLL(gymnet.LIB_PATH), EXPORT)
    header = re.sub(r"/\*.*?\*/", " ", _read("include", "gymnet_amd.h"), flags=re.S)
    assert _arity(header, r"\bint\s+" + EXPORT + r"\s*\(") == ARITY
    assert len(gymnet._capi.PROTOTYPES[EXPORT][1]) == ARITY
    assert _arity(_read("gym.net_amd", "csharp", "Native.cs"), r"extern int " + EXPORT + r"\(") == ARITY
    assert _arity(_read("include", "gymnet_amd.hpp"), r"check\(" + EXPORT + r"\(") == ARITY
    assert _arity(_read("gym.net_amd", "csharp", "VectorEnv.cs"), r"Native\." + EXPORT + r"\(") == ARITY
    assert ("void " + METHOD + "(") in _read("include", "gymnet_amd.hpp") and ("public void " + METHOD + "(") in _read("gym.net_amd", "csharp", "VectorEnv.cs")
    assert callable(importlib.import_module(gymnet.__name__ + ".vector_env").Actor.BoxPolicyGradient)


def test_box_gradient_arguments_are_checked_before_any_native_call(gymnet):
    """BoxPolicyGradient's refusals that need no device: the kind, and the rows under the Box names (float32 actions, logd_old, logd)"""
    import numpy as np
    import pytest
    from test_actor_grad_host import NoNativeCalls, _Tensor
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")
    N, m, W, count = 12, 7, 8, 90
    env = ve.VectorEnv.__new__(ve.VectorEnv)
    env.__dict__.update(_lib=NoNativeCalls(), _h=1, _owns_handle=False, NumberOfEnvironments=N, Device=0)

    def actor(box):
        o = ve.Actor.__new__(ve.Actor)
        o.__dict__.update(IsBox=box, _lib=env._lib, _h=1, _env=env, Widths=(W, 9, 1), Count=count, CriticWidths=None, CriticCount=0)
        return o

    f = lambda *shape, **kw: _Tensor(shape, **kw)
    good = dict(net=f(count), x=f(m, W), actions=f(m), coef=f(m), logd_old=f(m), logd=f(m), grad=f(count))
    with pytest.raises(ValueError, match="Box"):
        actor(False).BoxPolicyGradient(**good)
    rows = (f(m, dtype="torch.float64"), f(m, dtype="torch.int32"), f(m + 1), f(m, cuda=False), f(m, contiguous=False), np.zeros(m, np.float32), 4096)
    for name in ("actions", "coef", "logd_old", "logd"):
        for value in rows:
            with pytest.raises(ValueError, match=r"\b%s\b" % name):
                actor(True).BoxPolicyGradient(**dict(good, **{name: value}))
    for name, value in (("net", f(count + 1)), ("x", f(m, W, strides=(W, 2))), ("grad", f(count, cuda=False))):
        with pytest.raises(ValueError, match=r"\b%s\b" % name):
            actor(True).BoxPolicyGradient(**dict(good, **{name: value}))


def test_additive_in_abi_6_and_a_null_handle_is_refused(gymnet):
    capi = gymnet._capi
    lib = capi.load_library()
    assert capi.ABI_VERSION == 6 == lib.gymnet_abi_version()
    assert lib.gymnet_vecenv_actor_box_policy_gradient(None, None, 0, None, 0, 0, None, None, None, 0.2, 0.0, None, None, None, None) == capi.ERR_INVALID_ARG
