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


def test_additive_in_abi_6_and_a_null_handle_is_refused(gymnet):
    capi = gymnet._capi
    lib = capi.load_library()
    assert capi.ABI_VERSION == 6 == lib.gymnet_abi_version()
    assert lib.gymnet_vecenv_actor_box_policy_gradient(None, None, 0, None, 0, 0, None, None, None, 0.2, 0.0, None, None, None, None) == capi.ERR_INVALID_ARG
