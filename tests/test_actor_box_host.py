"""CPU checks of the Box actor (no GPU): the recipe table of tests/_actor_box_forms.py against the actor_box_rollout_kernel forms in
actor_box.hip's gfx950 assembly, that unit's register budget (no scratch, two waves per SIMD or more), the two exports in the ctypes
mirror with the header's arity, actor_pack's refusal of a last layer that is not one wide, and the composition rule in NumPy on
hand-made words."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _actor_box_forms as box

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def box_kernels():
    """{kernel name: resources} of actor_box.hip compiled to gfx950 assembly with the product's flags (tools/kernel_resources.py)"""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "actor_box.s")
        r = subprocess.run([kernel_resources.HIPCC] + kernel_resources.FLAGS + [os.path.join(kernel_resources.CSRC, "actor_box.hip"), "-o", out],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return kernel_resources.kernels(out)


@pytest.mark.timeout(900)
def test_forms_table_names_every_compiled_box_rollout_kernel(box_kernels):
    compiled = sorted(n for n in box_kernels if n.startswith("actor_box_rollout_kernel<"))
    table = sorted(row["kernel"] for row in box.FORMS)
    assert len(table) == len(set(table)) == 12
    assert compiled == table, (sorted(set(compiled) - set(table)), sorted(set(table) - set(compiled)))
    for row in box.FORMS:                                     # each row says how to reach its kernel
        env, ar, extras, records = re.match(r"actor_box_rollout_kernel<(\w+),(\w+),(\w+),(\w+)>", row["kernel"]).groups()
        assert box.ENVS[env] == row["env"] and (ar == "true") == row["auto_reset"]
        assert (extras == "true", records == "true") == box.SHAPES[row["shape"]]


@pytest.mark.timeout(900)
def test_box_kernels_do_not_spill_and_keep_two_waves(box_kernels):
    names = sorted(box_kernels)
    assert {"actor_box_act_kernel<2>", "actor_box_act_kernel<3>", "actor_push_kernel<float,3>"} <= set(names)
    assert len(names) == 15
    for n in names:
        assert box_kernels[n]["scratch"] == 0, (n, box_kernels[n])
        assert box_kernels[n]["occupancy"] >= 2, (n, box_kernels[n])


def test_the_unit_and_its_header_are_build_inputs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    assert "actor_box.hip" in kernel_resources._BUILD.SOURCES and "actor.hip" in kernel_resources._BUILD.SOURCES
    assert "actor_net.hpp" in kernel_resources._BUILD.DEPS and "actor_box.hip" in kernel_resources._BUILD.DEPS


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


def test_capi_declares_the_box_actor_exports_with_the_headers_arity(gymnet):
    import importlib
    capi = importlib.import_module(gymnet.__name__ + "._capi")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gymnet_amd.h")).read(), flags=re.S)
    for name in ("gymnet_vecenv_actor_box_config", "gymnet_vecenv_actor_box_act_device"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        assert name in capi.PROTOTYPES
        restype, argtypes = capi.PROTOTYPES[name]
        assert len(argtypes) == len(_split_args(m.group(1))) == 6, name
    assert capi.ABI_VERSION == 6


def test_pack_refuses_a_box_network_whose_last_layer_is_not_one_wide(gymnet):
    import importlib
    ve = importlib.import_module(gymnet.__name__ + ".vector_env")
    ok = [(np.zeros((5, 3), F32), np.zeros(5, F32)), (np.zeros((1, 5), F32), np.zeros(1, F32))]
    widths, flat = ve.actor_pack(ok, box=True)
    assert widths.tolist() == [3, 5, 1] and flat.size == 3 * 5 + 5 + 5 + 1
    two = [(np.zeros((5, 3), F32), np.zeros(5, F32)), (np.zeros((2, 5), F32), np.zeros(2, F32))]
    with pytest.raises(ValueError):
        ve.actor_pack(two, box=True)
    assert ve.actor_pack(two)[0].tolist() == [3, 5, 2]          # a Discrete network of that shape is fine

    class NoNativeCalls:                                        # VectorEnv.Actor on a Box env refuses it before any native call
        ActionSpace = ve.Box(np.array([-2], F32), np.array([2], F32), dtype=F32)
        ObsDim = 3

        def __getattr__(self, name):
            raise AssertionError("native call: " + name)
    with pytest.raises(ValueError):
        ve.Actor(NoNativeCalls(), two, 1)


@pytest.mark.parametrize("eps", [0.0, 0.3, 1.0])
def test_coin_at_below_and_above_the_threshold(eps):
    thr = box.coin_threshold(eps)
    assert thr == {0.0: 0xFF, 1.0: 0xFFFFFFFF}.get(eps, (int(np.floor(np.float64(F32(0.3)) * 2 ** 24)) << 8) | 0xFF)
    words_b = np.array([max(thr - 1, 0), thr, min(thr + 1, 0xFFFFFFFF)], np.uint32)
    words_a = np.array([0, 0x80000000, 0xFFFFFFFF], np.uint32)
    raw = np.array([0.25, -0.5, 0.75], F32)
    act, explore = box.compose(raw, words_a, words_b, eps, -1.0, 1.0)
    assert explore.tolist() == [True, True, eps == 1.0]
    # the threshold is the coin u01_24(b) <= epsilon itself
    assert np.array_equal(explore, box.u01_24(words_b) <= F32(eps))
    drawn = box.sample(words_a, -1.0, 1.0)
    assert drawn.tolist() == [-1.0, 0.0, float(F32(-1) + F32(2) * F32((2 ** 24 - 1) / 2 ** 24))]
    assert np.array_equal(act, np.where(explore, drawn, raw))


@pytest.mark.parametrize("low,high", [(-2.0, 2.0), (-1.0, 1.0)])
def test_clamp_below_inside_above_and_on_the_bounds(low, high):
    below, above = np.nextafter(F32(low), F32(-np.inf)), np.nextafter(F32(high), F32(np.inf))
    raw = np.array([-1e30, below, low, np.nextafter(F32(low), F32(0)), -0.0, 0.5, np.nextafter(F32(high), F32(0)), high, above, np.inf, np.nan], F32)
    got = box.clamp(raw, low, high)
    want = np.array([low, low, low, raw[3], -0.0, 0.5, raw[6], high, high, high, np.nan], F32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))            # bit patterns: -0.0 and the NaN pass unchanged
    act, explore = box.compose(raw, np.zeros(len(raw), np.uint32), np.full(len(raw), 0xFFFFFFFF, np.uint32), 0.3, low, high)
    assert not explore.any() and np.array_equal(act.view(np.uint32), want.view(np.uint32))
