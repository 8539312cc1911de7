"""CPU check of the advantage unit's compiled kernels (no GPU): gym.net_amd/csrc/advantage.hip compiled to gfx950 assembly with the
product's flags (tools/kernel_resources.py).  The compiled kernel set equals the table of tests/_advantage_forms.py, no kernel uses scratch
or LDS, and every one keeps at least 4 waves per SIMD (the heaviest form, V = 1 with values and boot at U = 8 rows in flight, holds 8 x 4
row registers and eight rows of 64-bit addresses: 120 VGPRs, 4 waves; V = 4 with values and boot at U = 4: 72 VGPRs, 7 waves)."""
import os
import re
import sys

import pytest

import _advantage_forms as forms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    return kernel_resources.collect(("advantage.hip",))


@pytest.mark.timeout(900)
def test_forms_table_names_every_compiled_advantage_kernel(kernels):
    table = sorted(row["kernel"] for row in forms.FORMS)
    assert len(table) == len(set(table)) == 8                      # V in {1, 4} x has_value x has_boot, nothing more
    assert sorted(kernels) == table, (sorted(set(kernels) - set(table)), sorted(set(table) - set(kernels)))
    for row in forms.FORMS:                                        # each row says how to reach its kernel
        vec, values, boot = re.match(r"advantage_kernel<(\d),(\w+),(\w+)>", row["kernel"]).groups()
        assert (int(vec), values == "true", boot == "true") == (row["vec"], row["values"], row["boot"])
        reach = row["reach"]
        stride = reach["count"] + reach["pad"]
        assert forms.kernel_for(reach["count"], stride, reach["offset"] % 4 == 0, row["values"], row["boot"]) == row["kernel"]


@pytest.mark.timeout(900)
def test_no_advantage_kernel_uses_scratch_and_each_keeps_four_waves(kernels):
    for name in sorted(kernels):
        k = kernels[name]
        print(f"{name:40s} VGPRs {k['vgpr']:3d}  waves {k['occupancy']}  scratch {k['scratch']}  LDS {k['lds']}")
        assert k["scratch"] == 0 and k["lds"] == 0, (name, k)
        assert k["occupancy"] >= 4, (name, k)


def test_the_tables_constants_are_the_units():
    src = open(os.path.join(ROOT, "gym.net_amd", "csrc", "advantage.hip")).read()
    m = re.search(r"static constexpr int U = V == 4 \? (\d+) : (\d+);", src)
    assert m and {4: int(m.group(1)), 1: int(m.group(2))} == forms.U
    hpp = open(os.path.join(ROOT, "gym.net_amd", "csrc", "advantage.hpp")).read()
    m = re.search(r"constexpr int64_t kAdvantageNarrowBelow = ([0-9 *]+);", hpp)
    assert m and eval(m.group(1)) == forms.NARROW_BELOW
    assert "__restrict__" not in re.sub(r"//.*", "", src)          # the outputs may alias the inputs
