"""Where the headline kernel waits for the action, read from the assembly the product's flags produce (no GPU, about a minute of hipcc; the
route walker of tests/test_step_fastpath_asm.py).  The action slice is the one input of a launch that no earlier launch left in the
Infinity Cache, so it arrives last; the full-workgroup body (csrc/step_kernels.hpp step_body_wg) therefore runs everything the action has
no part in — CartPole::step_pre of the four sub-lanes, the float64 done flags, the reset's draw — in front of the wait for it, and only
CartPole::step_post behind it (docs/ledger.md §28).  Asserted on the route a full wave takes with small angles and 1..64 finished slots:

  1. the action load is the fifth global_load_dwordx4, its base built from the kernel's second argument (user SGPRs s[4:5]: the kernarg
     segment pointer takes s[0:1], `state` s[2:3]);
  2. at least 100 VALU instructions run before the first instruction that reads one of its four destination registers (the code before the
     split had the compare `action == 1` a dozen instructions into the arithmetic).  The floor is the source's: 4 x 20 action-free
     instructions of the dynamics + 34 for the flags = 114; the count found is printed;
  3. no store is issued ahead of that first read: with loads and stores both in flight the compiler can only wait for everything
     (ledger §4), and the wait for the action would cover the stores too;
  4. the wait that covers the action load is the last vmcnt wait in front of the stores."""
import os
import re
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_step_fastpath_asm as F  # noqa: E402  (route, _function_lines; only the module object is imported)

ROOT = F.ROOT
VALU_BEFORE_ACTION_FLOOR = 100
LOAD = re.compile(r"global_load_dwordx4 v\[(\d+):(\d+)\], v\d+, s\[(\d+):(\d+)\]")


def _vgprs(text):
    got = set()
    for a, b in re.findall(r"v\[(\d+):(\d+)\]", text):
        got |= set(range(int(a), int(b) + 1))
    got |= {int(a) for a in re.findall(r"\bv(\d+)\b", text)}
    return got


def _reads(line):
    """VGPRs an instruction reads: every operand of a store, LDS write or compare, every operand but the first of anything else"""
    if " " not in line:
        return set()
    op, rest = line.split(None, 1)
    parts = [p.strip() for p in rest.split(",")]
    if op.startswith(("global_store", "flat_store", "ds_write", "scratch_store", "buffer_store")):
        return _vgprs(rest)
    if op.startswith("v_cmp"):                      # the destination is a mask (vcc or an SGPR pair), never a VGPR
        return _vgprs(rest)
    if op.startswith("s_"):
        return set()
    return _vgprs(",".join(parts[1:]))


@pytest.fixture(scope="module")
def action_use():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    with tempfile.TemporaryDirectory() as d:
        path = kernel_resources.assembly("cartpole", d)
        lines = F._function_lines(path, F.HEADLINE)
    _, ins = F.route(lines)
    loads = [i for i, l in enumerate(ins) if l.startswith("global_load")]
    assert len(loads) == 5 and all(LOAD.match(ins[i]) for i in loads), [ins[i] for i in loads]
    at = loads[4]
    m = LOAD.match(ins[at])
    dst = set(range(int(m.group(1)), int(m.group(2)) + 1))
    assert len(dst) == 4
    use = next((i for i in range(at + 1, len(ins)) if _reads(ins[i]) & dst), None)
    assert use is not None, "nothing on the route reads the action"
    return ins, at, (int(m.group(3)), int(m.group(4))), use


@pytest.mark.timeout(900)
def test_the_fifth_load_is_the_action(action_use):
    ins, at, (lo, hi), _ = action_use
    add = next(l for l in reversed(ins[:at]) if re.match(rf"s_add_u32 s{lo},", l))
    addc = next(l for l in reversed(ins[:at]) if re.match(rf"s_addc_u32 s{hi},", l))
    assert re.search(r"\bs4\b", add) and re.search(r"\bs5\b", addc), (add, addc, ins[at])


@pytest.mark.timeout(900)
def test_the_action_is_first_read_behind_the_action_free_work(action_use):
    ins, at, _, use = action_use
    before = sum(1 for l in ins[:use] if l.startswith("v_"))
    print("VALU in front of the first read of the action:", before, "| first read:", ins[use])
    assert before >= VALU_BEFORE_ACTION_FLOOR, (before, ins[use])


@pytest.mark.timeout(900)
def test_no_store_is_issued_ahead_of_the_action(action_use):
    ins, _, _, use = action_use
    early = [l for l in ins[:use] if l.startswith(("global_store", "flat_"))]
    assert not early, early


@pytest.mark.timeout(900)
def test_the_wait_for_the_action_is_the_last_vmcnt_wait_before_the_stores(action_use):
    ins, at, _, use = action_use
    # the action is the last load issued and no store is in flight: the wait that covers it is the vmcnt(0) nearest in front of its first read
    waits = [i for i in range(at + 1, use + 1) if ins[i].startswith("s_waitcnt") and "vmcnt" in ins[i]]
    assert waits and re.search(r"vmcnt\(0\)", ins[waits[-1]]), [ins[i] for i in waits]
    cover = waits[-1]
    first_store = next(i for i, l in enumerate(ins) if l.startswith("global_store"))
    assert cover < first_store
    later = [ins[i] for i in range(cover + 1, first_store) if ins[i].startswith("s_waitcnt") and "vmcnt" in ins[i]]
    assert not later, later
