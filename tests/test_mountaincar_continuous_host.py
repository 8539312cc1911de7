"""MountainCarContinuous-v0 without a GPU: the ABI's description of the env, the C# enum, the two CPU twins against each other on the
golden states, and the env's compiled kernel set (csrc/env_mountaincar_continuous.hip, gfx950 assembly) against its recipe table
(tests/_mountaincar_continuous_matrix.py) with the register budget the launch policy relies on."""
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _mountaincar_continuous_matrix as MC  # noqa: E402
import _mountaincar_continuous_twin as tw  # noqa: E402
from test_instantiation_coverage import FAMILIES, check_coverage  # noqa: E402

ENV_ID = 4


def test_env_description(gymnet):
    assert gymnet.ENV_IDS["MountainCarContinuous-v0"] == ENV_ID
    i = gymnet.env_describe(ENV_ID)
    assert i.env_id == ENV_ID and i.name == b"MountainCarContinuous-v0"
    assert i.state_dim == 2 and i.obs_dim == 2 and i.obs_aliases_state == 1
    assert i.action_is_box == 1 and i.action_n == 0 and (i.action_low, i.action_high) == (-1.0, 1.0)
    assert list(i.obs_low[:2]) == [np.float32(-1.2), np.float32(-0.07)] and list(i.obs_high[:2]) == [np.float32(0.6), np.float32(0.07)]
    assert i.reward_low == -math.inf and i.reward_high == 100.0
    # 8 B state read + 4 B action + 8 B state written + 4 B reward + 1 B done, like MountainCar; nothing stored twice
    assert i.algorithmic_bytes_per_step == i.traffic_bytes_per_step == 25 == gymnet.env_describe(2).algorithmic_bytes_per_step
    assert set(i.state_row_in_obs) == {-1}
    with pytest.raises(ValueError):
        gymnet.env_describe(ENV_ID + 1)
    assert issubclass(gymnet.MountainCarContinuousEnv, gymnet.GpuEnv) and gymnet.MountainCarContinuousEnv.ENV == "MountainCarContinuous-v0"
    assert "MountainCarContinuousEnv" in gymnet.__all__


def test_header_csharp_and_python_agree_on_the_env_id():
    hdr = open(os.path.join(ROOT, "include", "gymnet_amd.h")).read()
    assert re.search(r"GYMNET_ENV_MOUNTAINCAR_CONTINUOUS\s*=\s*(\d+)", hdr).group(1) == str(ENV_ID)
    assert re.search(r"#define GYMNET_ABI_VERSION 6\b", hdr)                       # an added enum value is a compatible addition
    native = open(os.path.join(ROOT, "gym.net_amd", "csharp", "Native.cs")).read()
    assert re.search(r"enum GymnetEnvId \{[^}]*\bMountainCarContinuous = (\d+)", native).group(1) == str(ENV_ID)
    code = re.sub(r"//.*", "", open(os.path.join(ROOT, "gym.net_amd", "csharp", "GpuEnv.cs")).read())
    m = re.search(r"public sealed class GpuMountainCarContinuousEnv\s*:\s*GpuEnv\s*\{([^}]*)\}", code)
    assert m and "base(GymnetEnvId.MountainCarContinuous," in m.group(1)
    assert "validateActions" not in m.group(1)                                       # a Box env: nothing to validate, like GpuPendulumEnv


def test_float32_twin_stays_within_1e6_of_the_float64_restatement(golden, oracle):
    g = golden("mountaincar_continuous")
    s, rw, d = tw.step_f32(g["state"], g["action"])
    assert np.abs(s.astype(np.float64) - g["next_state"]).max() <= 1e-6
    assert np.abs(rw.astype(np.float64) - g["reward"]).max() <= 1e-5
    near = np.abs(g["next_state"][0] - 0.45) < 1e-6
    assert np.array_equal(d[~near], g["done"].astype(bool)[~near])
    # and the restatement is the fixture: regenerating it gives the same numbers
    ns, rw64, d64 = tw.step_f64(g["state"].astype(np.float64), g["action"].astype(np.float64))
    assert np.array_equal(ns, g["next_state"]) and np.array_equal(rw64, g["reward"]) and np.array_equal(d64, g["done"].astype(bool))
    # the fixture covers what it claims: both velocity clips, the left wall, the right clip, the goal, out-of-range actions
    assert (g["next_state"][1] == 0.07).any() and (g["next_state"][1] == -0.07).any()
    wall = (g["next_state"][0] == -1.2)
    assert wall.any() and (g["next_state"][1][wall] == 0.0).all()
    assert (g["next_state"][0] == 0.6).any() and g["done"].sum() > 100 and (g["done"] == 0).sum() > 100
    assert (np.abs(g["action"]) > 1).sum() > 100


def test_goal_threshold_is_the_float64_comparison():
    """0x3EE66667 is the smallest float32 >= 0.45: for float32 positions the kernel's `p >= GOAL` is upstream's float64 `p >= 0.45`."""
    assert float(tw.BELOW_GOAL32) < 0.45 <= float(tw.GOAL32)
    assert np.float32(0.45) == tw.BELOW_GOAL32                                       # 0.45f itself lies below 0.45
    hpp = open(os.path.join(ROOT, "gym.net_amd", "csrc", "envs.hpp")).read()
    assert float.fromhex(re.search(r"GOAL = (0x[0-9a-fp.+-]+)f;", hpp).group(1)) == float(tw.GOAL32)
    bits = np.arange(0x3EE66600, 0x3EE66700, dtype=np.uint32).view(np.float32)
    assert np.array_equal(bits >= tw.GOAL32, bits.astype(np.float64) >= 0.45)


def _compiled():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    import kernel_resources
    return kernel_resources.collect(("mountaincar_continuous",))


@pytest.fixture(scope="module")
def compiled():
    return _compiled()


@pytest.mark.timeout(900)
def test_recipe_table_equals_the_compiled_instantiation_set(compiled):
    recipes = MC.recipes()
    names = [r["name"] for r in recipes]
    assert len(names) == len(set(names))
    missing, stale, unexplained = check_coverage(set(compiled), recipes, MC.EXCLUDED)
    assert not missing, f"compiled instantiations without a recipe: {missing}"
    assert not stale, f"recipes naming no compiled instantiation: {stale}"
    assert not unexplained, f"compiled kernels neither in the table nor excluded: {unexplained}"
    assert set(MC.EXCLUDED) <= set(compiled)
    assert {r["family"] for r in recipes} == {"step_kernel", "rollout_kernel", "resident_kernel"} and set(FAMILIES) >= {r["family"] for r in recipes}


@pytest.mark.timeout(900)
def test_register_budget(compiled):
    for name, v in compiled.items():
        if name.startswith("step_kernel"):
            assert v["scratch"] == 0, (name, v)                                      # no step kernel spills
        if name.startswith("rollout_kernel<MountainCarContinuous,4,"):
            assert v["occupancy"] >= 4 and v["scratch"] <= 160, (name, v)            # 2^20 lanes = 4096 four-lane waves: four per SIMD


def test_recipes_meet_the_preconditions_of_their_form():
    per_family = {}
    for r in MC.recipes():
        per_family.setdefault(r["family"], []).append(r)
        n, fam = r["n"], r["family"]
        assert r["env"] == "MountainCarContinuous" and r["name"].startswith(fam + "<MountainCarContinuous,")
        if fam == "step_kernel":
            v, lanes = r["vec"], r["block"] * r["vec"]
            assert n > lanes and n % lanes != 0 and (v == 1 or n % v != 0) and n % (64 * v) != 0, r["name"]
        elif fam == "rollout_kernel":
            v = r["vec"]
            name, got_v = MC.rollout_instantiation(r["launch"]["vec"], n, r["auto_reset"], r["name"].split(",")[3] == "true", r["actions"],
                                                   r["records"] != "none", r["records"] == "no_overflow", r["launch"]["reset_form"],
                                                   action_stride=r["action_stride"])
            assert name == r["name"] and got_v == v
            assert r["actions"] in ("ring", "sample")                                 # epsilon-greedy is Discrete-only
            if v > 1:
                assert n % v == 0 and n % (MC.M.ROLLOUT_BLOCK * v) != 0 and n > MC.M.ROLLOUT_BLOCK * v, r["name"]
            else:
                assert n % 4 != 0, r["name"]
            if r["records"] != "none":
                assert r["episode_stats"], r["name"]
        else:
            assert 1 <= n <= 64 and not r["done_list"] and not r["final_obs"], r["name"]
        targs = r["name"].split("<")[1].rstrip(">").split(",")
        ex_pos = 2 if fam == "resident_kernel" else 3
        ex = r["done_list"] or r["episode_stats"] or r["final_obs"] or r["lane_seeds"]
        assert (targs[ex_pos] == "true") == bool(ex) and (targs[ex_pos - 1] == "true") == r["auto_reset"], r["name"]
    for fam, rs in per_family.items():
        offs = {r["lane_offset"] for r in rs}
        assert 0 in offs and {o % 4 for o in offs} >= {1, 2, 3} and max(offs) >= 1 << 32, fam
    # the combinations no other env reaches: Box actions with auto-reset and records, sampled actions on finishing lanes, a time limit
    rs = per_family["rollout_kernel"]
    assert any(r["auto_reset"] and r["records"] != "none" for r in rs) and any(r["actions"] == "sample" and r["auto_reset"] for r in rs)
    assert any(r["max_episode_steps"] for r in rs) and any(r["max_episode_steps"] for r in per_family["step_kernel"])
