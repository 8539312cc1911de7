"""CPU checks of gymnet_vecenv_actor_policy_gradient / _value_gradient: exported, one arity in every binding, additive in ABI 6, refused on
a null handle, built from csrc/actor_grad.hip / .hpp.  Every test fails without the feature: the exports do not exist."""
import ctypes
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def test_additive_in_abi_6_a_null_handle_is_refused_and_the_unit_is_a_build_input(gymnet):
    capi, build = gymnet._capi, importlib.import_module(gymnet.__name__ + ".build")
    lib = capi.load_library()
    assert capi.ABI_VERSION == 6 == lib.gymnet_abi_version()
    assert "actor_grad.hip" in build.SOURCES and "actor_grad.hip" in build.DEPS and "actor_grad.hpp" in build.DEPS
    assert lib.gymnet_vecenv_actor_policy_gradient(None, None, 0, None, 0, 0, None, None, None, 0.2, 0.0, None, None, None) == capi.ERR_INVALID_ARG
    assert lib.gymnet_vecenv_actor_value_gradient(None, None, 0, None, 0, 0, None, None, None, None) == capi.ERR_INVALID_ARG

