"""The recipe table (tests/_instantiation_matrix.py) covers the compiled kernel set exactly, asserted from the gfx950 assembly (no GPU):
every step_kernel*, rollout_kernel and resident_kernel instantiation the five env_*.hip units compile has a recipe that
tests/test_gpu_instantiation_matrix.py runs against the oracle, and every recipe names a kernel that exists.  A new instantiation
without a recipe fails here by name.  Also the preconditions of the form each recipe claims (wide rollouts n % w == 0, the
producer / consumer kernel whole 512-lane tiles, the strict lane-pair kernel whole groups).  ~1 minute of hipcc."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _instantiation_matrix as M  # noqa: E402

FAMILIES = ("step_kernel", "step_kernel_pipe", "step_kernel_pipe2", "step_kernel_lds", "rollout_kernel", "resident_kernel")


def _kernel_text(asm_name):
    """The assembly's name as kernel_text prints it: step_kernel_lds carries its default computing-wave count (8) as a fifth argument."""
    m = re.match(r"^(step_kernel_lds<.*),(\d+)>$", asm_name)
    if m:
        assert m.group(2) == "8", asm_name                      # the only count select_step launches
        return m.group(1) + ">"
    return asm_name


def check_coverage(compiled, recipes, excluded):
    """(missing, stale, unexplained) kernel names: compiled without a recipe, recipes without a kernel, compiled kernels that are
    neither recipes nor excluded."""
    launched = {_kernel_text(k) for k in compiled if k.split("<")[0] in FAMILIES}
    others = {k for k in compiled if k.split("<")[0] not in FAMILIES}
    names = [r["name"] for r in recipes]
    return sorted(launched - set(names)), sorted(set(names) - launched), sorted(others - set(excluded))


@pytest.mark.timeout(900)
def test_recipe_table_equals_the_compiled_instantiation_set():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    import kernel_resources
    compiled = set(kernel_resources.collect())
    recipes = M.recipes()
    names = [r["name"] for r in recipes]
    assert len(names) == len(set(names)), sorted({n for n in names if names.count(n) > 1})
    missing, stale, unexplained = check_coverage(compiled, recipes, M.EXCLUDED)
    assert not missing, f"compiled instantiations without a recipe: {missing}"
    assert not stale, f"recipes naming no compiled instantiation: {stale}"
    assert not unexplained, f"compiled kernels neither in the table nor excluded: {unexplained}"
    assert set(M.EXCLUDED) <= compiled, sorted(set(M.EXCLUDED) - compiled)
    for name, why in M.EXCLUDED.items():
        path = os.path.join(ROOT, why.split(" ")[0])
        assert os.path.exists(path), (name, why)                 # each exclusion cites a test that exists


def test_recipes_meet_the_preconditions_of_their_form():
    recipes = M.recipes()
    per_family = {}
    for r in recipes:
        per_family.setdefault(r["family"], []).append(r)
        n, fam = r["n"], r["family"]
        assert r["name"].startswith(fam + "<") and r["name"].split("<")[1].split(",")[0] == r["env"], r["name"]
        if fam == "step_kernel":
            v, lanes = r["vec"], r["block"] * r["vec"]
            assert n > lanes and n % lanes != 0, r["name"]                            # a full workgroup and a partial last one
            assert v == 1 or n % v != 0, r["name"]                                    # a thread with fewer than V lanes
            assert (n % (64 * v)) != 0, r["name"]                                     # a partial last wave
        elif fam == "step_kernel_pipe":
            assert n % (256 * r["items"]) != 0 and n > 256 * r["items"], r["name"]
        elif fam == "step_kernel_lds":
            tiles = n // M.LDS_TILE
            assert n % M.LDS_TILE == 0 and tiles > r["items"] and tiles % r["items"] != 0, r["name"]
        elif fam == "step_kernel_pipe2":
            group = 2 * r["items"] * r["block"]
            if r["any_n"]:
                assert n % group != 0 and n % 2 == 0 and n % 64 != 0, r["name"]      # ragged: the deferred-reset form's guarded tail
            else:
                assert n % (2 * r["items"] * 256) == 0 and n // group >= 2, r["name"]  # strict: whole groups only (select_step counts 256-thread groups)
        elif fam == "rollout_kernel":
            v = r["vec"]
            name, got_v = M.rollout_instantiation(r["env"], r["launch"]["vec"], n, r["auto_reset"], r["name"].split(",")[3] == "true",
                                                  r["actions"], r["records"] != "none", r["records"] == "no_overflow",
                                                  r["launch"].get("reset_form", 0), action_stride=r["action_stride"])
            assert name == r["name"] and got_v == v, (name, r["name"])
            if v > 1:
                assert n % v == 0 and n % (M.ROLLOUT_BLOCK * v) != 0 and n > M.ROLLOUT_BLOCK * v, r["name"]
                assert r["action_stride"] is None or r["action_stride"] % v == 0, r["name"]
            else:
                assert n % 4 != 0, r["name"]                                           # the narrow form gets a ragged batch
            if r["records"] != "none":
                assert r["episode_stats"], r["name"]
        elif fam == "resident_kernel":
            assert 1 <= n <= 64 and not r["done_list"] and not r["final_obs"], r["name"]
        ex = r["done_list"] or r["episode_stats"] or r["final_obs"] or r["lane_seeds"]
        if fam in ("step_kernel", "rollout_kernel", "resident_kernel"):
            targs = r["name"].split("<")[1].rstrip(">").split(",")
            ex_pos = {"step_kernel": 3, "rollout_kernel": 3, "resident_kernel": 2}[fam]
            ar_pos = ex_pos - 1
            assert (targs[ex_pos] == "true") == bool(ex) and (targs[ar_pos] == "true") == r["auto_reset"], r["name"]
        else:
            assert not ex, r["name"]                                                   # the multi-lane forms are lean only
    # lane offsets of every family: 0, each of 1..3 mod 4, and one >= 2^32
    for fam, rs in per_family.items():
        offs = {r["lane_offset"] for r in rs}
        assert 0 in offs and {o % 4 for o in offs} >= {1, 2, 3} and max(offs) >= 1 << 32, fam
    assert set(per_family) == set(FAMILIES)


def test_a_missing_or_stale_recipe_is_named():
    """The comparison itself: dropping one recipe or adding a fake one is reported by kernel name."""
    recipes = M.recipes()
    compiled = {r["name"] for r in recipes} | set(M.EXCLUDED)
    compiled = {n[:-1] + ",8>" if n.startswith("step_kernel_lds<") else n for n in compiled}
    assert check_coverage(compiled, recipes, M.EXCLUDED) == ([], [], [])
    gone = recipes[17]["name"]
    assert check_coverage(compiled, recipes[:17] + recipes[18:], M.EXCLUDED)[0] == [gone]
    fake = dict(recipes[0], name="step_kernel<CartPole,8,true,false,15,1>")
    assert check_coverage(compiled, recipes + [fake], M.EXCLUDED)[1] == [fake["name"]]
