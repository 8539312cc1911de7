"""The headline kernel's shortened chain, read from the assembly the product's flags produce (docs/ledger.md §38; no GPU, about a minute of
hipcc; the route walker of tests/test_step_fastpath_asm.py).  On the route a wave of a full workgroup takes with small angles, 1..64
finished slots and no sub-lane near a threshold:

  1. no float64 instruction: the done flags are float32 compares against the band's four constants (csrc/cartpole_done_filter.hpp), and
     the binary64 compares exist in the kernel but are reached only through the branch taken when some sub-lane is ambiguous;
  2. fewer instructions in front of the first global_load than the parent had, all of them scalar but the thread's own offsets, and no
     vector compare or exec-mask branch among them (the full-workgroup guard is a scalar compare; the tick writer sits behind the body).

The draw's slot read (ds_read_b32) is still followed at once by its wait: covering it measured no gain on the parent (the `slot` ceiling of
profiles/step_chain.txt is inside the noise, on the wrong side of zero), so by the rule set beforehand it was not built and is not asserted."""
import os
import re
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
# the route walker's count on the parent commit 56b4e52 ("Box actor: record the action's log-density and the critic's value"): its first
# global_load_dwordx4 is instruction 45 of the route (0-based), so 45 instructions stand in front of it
PARENT_BEFORE_FIRST_LOAD = 45
BAND = {"0x40199996": "x_lo", "0x4019999e": "x_hi", "0x3e56774c": "theta_lo", "0x3e567754": "theta_hi"}       # threshold -+ 4 float32 steps


@pytest.fixture(scope="module")
def headline():
    import test_step_fastpath_asm as F
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    import kernel_resources
    with tempfile.TemporaryDirectory() as d:
        lines = F._function_lines(kernel_resources.assembly("cartpole", d), F.HEADLINE)
    blocks = F._blocks(lines)
    _, ins = F.route(lines)
    return blocks, ins


@pytest.mark.timeout(900)
def test_band_constants_are_the_thresholds_plus_and_minus_four_steps():
    import numpy as np
    for thr, lo, hi in ((2.4, "x_lo", "x_hi"), (0.20943951606750488, "theta_lo", "theta_hi")):
        b = int(np.array([thr], np.float32).view(np.uint32)[0])
        assert {"0x%08x" % (b - 4): lo, "0x%08x" % (b + 4): hi}.items() <= BAND.items()


@pytest.mark.timeout(900)
def test_no_float64_on_the_common_route_and_the_exact_compares_behind_the_ambiguous_branch(headline):
    blocks, ins = headline
    assert not [l for l in ins if "_f64" in l], [l for l in ins if "_f64" in l]
    # the float32 filter is on the route: 3 compares per term, 2 terms, 4 sub-lanes, against the band's constants (held in SGPRs)
    consts = {}
    for l in ins:
        m = re.match(r"s_mov_b32 (s\d+), (0x[0-9a-f]+)", l)
        if m and m.group(2) in BAND:
            consts[m.group(1)] = BAND[m.group(2)]
    assert sorted(consts.values()) == sorted(BAND.values()), consts
    filt = [k for k, l in enumerate(ins) if re.match(r"v_cmp_[lg]t_f32_e64 s\[\d+:\d+\], \|v\d+\|, (s\d+)$", l) and l.rsplit(" ", 1)[1] in consts]
    assert len(filt) == 24, [ins[k] for k in filt]
    # the first scalar branch behind the last of them leaves the route for the binary64 compares: 2 terms x 4 sub-lanes
    k = next(k for k in range(filt[-1], len(ins)) if ins[k].startswith("s_cbranch"))
    assert ins[k].startswith("s_cbranch_scc"), ins[k]
    at = {x: i for i, b in enumerate(blocks) for x in b["labels"]}
    target = at[ins[k].split()[-1]]
    assert sum(1 for l in blocks[target]["ins"] if l.startswith("v_cmp_gt_f64")) == 8, blocks[target]["ins"]
    # ... and that block is entered from nowhere else: it has no label another branch names and the block in front of it does not fall into it
    label = ins[k].split()[-1]
    users = [l for b in blocks for l in b["ins"] if l.startswith(("s_branch", "s_cbranch")) and l.split()[-1] == label]
    assert len(users) == 1 and len(blocks[target]["labels"]) == 1, (users, blocks[target]["labels"])
    assert blocks[target - 1]["ins"][-1].startswith(("s_branch", "s_endpgm")), blocks[target - 1]["ins"][-1]


@pytest.mark.timeout(900)
def test_fewer_instructions_in_front_of_the_first_load_and_none_of_them_a_vector_compare(headline):
    _, ins = headline
    first = next(k for k, l in enumerate(ins) if l.startswith("global_load"))
    head = ins[:first]
    print("instructions in front of the first global_load:", first, "(parent: %d)" % PARENT_BEFORE_FIRST_LOAD)
    assert first < PARENT_BEFORE_FIRST_LOAD, head
    assert not [l for l in head if l.startswith(("v_cmp", "s_and_saveexec", "s_cbranch_execz", "s_waitcnt"))], head
    assert [l for l in head if re.match(r"s_cmp_[lg]t_i32 ", l)] and [l for l in head if l.startswith("s_cbranch_scc")], head      # the scalar guard
    assert sum(1 for l in head if l.startswith("v_")) <= 4, head                                       # the thread's offsets, nothing else
    # the five loads leave within a dozen instructions of each other, the row bases formed between them by adds (no 64-bit multiply chain)
    loads = [k for k, l in enumerate(ins) if l.startswith("global_load")]
    assert len(loads) == 5 and loads[-1] - loads[0] <= 12, loads
    assert not [l for l in ins[first:loads[-1]] if l.startswith("s_mul")], ins[first:loads[-1]]
