"""CPU checks of gymnet_vecenv_actor_apply_gradient: exported, one arity in every binding, additive in ABI 6, refused on a null handle,
built from csrc/actor_optim.hip / .hpp.  Every test fails without the feature: the export does not exist."""
import ctypes
import importlib
import re

from test_actor_grad_host import _arity, _read         # the parameter count of a declaration or call; a file of the repository

EXPORT, METHOD, ARITY = "gymnet_vecenv_actor_apply_gradient", "ActorApplyGradient", 14


def test_one_arity_in_every_binding(gymnet):
    assert hasattr(ctypes.CDLL(gymnet.LIB_PATH), EXPORT)
    header = re.sub(r"/\*.*?\*/", " ", _read("include", "gymnet_amd.h"), flags=re.S)
    assert _arity(header, r"\bint\s+" + EXPORT + r"\s*\(") == ARITY
    assert [int(re.search(r"#define\s+GYMNET_OPT_" + n + r"\s+(\d+)", header).group(1)) for n in ("SGD", "ADADELTA", "ADAM")] == [0, 1, 2]
    assert len(gymnet._capi.PROTOTYPES[EXPORT][1]) == ARITY
    assert _arity(_read("gym.net_amd", "csharp", "Native.cs"), r"extern int " + EXPORT + r"\(") == ARITY
    assert _arity(_read("include", "gymnet_amd.hpp"), r"check\(" + EXPORT + r"\(") == ARITY
    assert _arity(_read("gym.net_amd", "csharp", "VectorEnv.cs"), r"Native\." + EXPORT + r"\(") == ARITY
    assert ("void " + METHOD + "(") in _read("include", "gymnet_amd.hpp") and ("public void " + METHOD + "(") in _read("gym.net_amd", "csharp", "VectorEnv.cs")
    assert callable(importlib.import_module(gymnet.__name__ + ".vector_env").Actor.ApplyGradient)


def test_an_unknown_rule_is_refused_before_any_native_call(gymnet):
    """the one refusal of ApplyGradient that needs no device (the handle's stream is asked for next)"""
    import pytest
    from test_actor_grad_host import NoNativeCalls
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")
    actor = ve.Actor.__new__(ve.Actor)
    actor.__dict__.update(_lib=NoNativeCalls(), _h=1, _env=None)
    for rule in ("rmsprop", "Adam", None, 2):
        with pytest.raises(ValueError, match="rule"):
            actor.ApplyGradient(None, None, None, rule=rule)


def test_additive_in_abi_6_a_null_handle_is_refused_and_the_unit_is_a_build_input(gymnet):
    capi, build = gymnet._capi, importlib.import_module(gymnet.__name__ + ".build")
    lib = capi.load_library()
    assert capi.ABI_VERSION == 6 == lib.gymnet_abi_version()
    assert "actor_optim.hip" in build.SOURCES and "actor_optim.hip" in build.DEPS and "actor_optim.hpp" in build.DEPS
    assert lib.gymnet_vecenv_actor_apply_gradient(None, 2, None, 1, None, None, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, None) == capi.ERR_INVALID_ARG
