"""CPU checks of gymnet_vecenv_actor_q_gradient: exported, one arity in every binding, additive in ABI 6, refused on a null handle, and
Actor.QGradient refusing a Box actor and missing rows before any native call.  Every test fails without the feature: the export does not exist."""
import ctypes
import importlib
import re

import pytest

from test_actor_grad_host import NoNativeCalls, _arity, _read

EXPORT, METHOD, ARITY = "gymnet_vecenv_actor_q_gradient", "ActorQGradient", 19


def test_one_arity_in_every_binding(gymnet):
    assert hasattr(ctypes.CDLL(gymnet.LIB_PATH), EXPORT)
    header = re.sub(r"/\*.*?\*/", " ", _read("include", "gymnet_amd.h"), flags=re.S)
    assert _arity(header, r"\bint\s+" + EXPORT + r"\s*\(") == ARITY
    assert len(gymnet._capi.PROTOTYPES[EXPORT][1]) == ARITY
    assert _arity(_read("gym.net_amd", "csharp", "Native.cs"), r"extern int " + EXPORT + r"\(") == ARITY
    assert _arity(_read("include", "gymnet_amd.hpp"), r"check\(" + EXPORT + r"\(") == ARITY
    assert _arity(_read("gym.net_amd", "csharp", "VectorEnv.cs"), r"Native\." + EXPORT + r"\(") == ARITY
    assert ("void " + METHOD + "(") in _read("include", "gymnet_amd.hpp") and ("public void " + METHOD + "(") in _read("gym.net_amd", "csharp", "VectorEnv.cs")
    assert callable(importlib.import_module(gymnet.__name__ + ".vector_env").Actor.QGradient)


def test_additive_in_abi_6_and_a_null_handle_is_refused(gymnet):
    capi = gymnet._capi
    lib = capi.load_library()
    assert capi.ABI_VERSION == 6 == lib.gymnet_abi_version()
    assert lib.gymnet_vecenv_actor_q_gradient(None, None, None, 0, None, 0, None, 0, 0, None, None, None, 0.99, 1.0, 0, None, None, None, None) == capi.ERR_INVALID_ARG


def test_a_box_actor_and_missing_rows_are_refused_before_any_native_call(gymnet):
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")
    env = ve.VectorEnv.__new__(ve.VectorEnv)
    env.__dict__.update(_lib=NoNativeCalls(), _h=1, _owns_handle=False, NumberOfEnvironments=12, Device=0)

    def actor(box):
        o = ve.Actor.__new__(ve.Actor)
        o.__dict__.update(IsBox=box, _lib=env._lib, _h=1, _env=env, Widths=(8, 9, 2), Count=101)
        return o

    with pytest.raises(ValueError, match="Discrete"):
        actor(True).QGradient(None, None, None, None, None, None)
    for missing in ("actions", "reward", "done"):
        with pytest.raises(ValueError, match="required"):
            actor(False).QGradient(**dict(dict.fromkeys(("net", "x", "x_next", "actions", "reward", "done"), 4096), **{missing: None}))
