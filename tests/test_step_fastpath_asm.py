"""The headline kernel's full-workgroup route, read from the assembly the product's flags produce (tools/kernel_resources.py FLAGS; no GPU,
about a minute of hipcc; the method of tests/test_step_args_preload.py).  step_kernel<CartPole,4,true,false,15,1> runs one lock-step
generation of waves at 2^20 lanes, so every vector instruction between the loads and the last store is exposed (docs/ledger.md §4, §25).
Asserted for the route a wave of a FULL workgroup takes when every pole angle is small and the wave holds 1..64 finished slots —
essentially every wave of the benchmark:

  1. the five loads and the six stores (reward, done, four state rows) take their address as `v_off, s[base:base+1]`: row bases on the
     scalar unit, one 32-bit offset per thread (csrc/lanes.hpp WgLanes);
  2. NumVgprs <= 64 (eight waves per SIMD);
  3. the VALU instructions from the kernel's entry to the last store number fewer than the 428 counted by hand before the change and no
     more than the 394 this walker counts after it (the same walker counts 425 on the code before the change: the hand count also
     entered the block in which ONE thread of the launch writes the next tick).  394 is a regression guard, not a target.

The route is found, not transcribed: the function is cut into basic blocks, and the route is the one with the fewest VALU instructions
from the entry through a block that parks a reset draw in LDS (ds_write_b128: the reset is run, not skipped) to the block that stores the
four state rows with scalar bases.  Three rules keep that search on what a full wave executes: the region behind the first
s_cbranch_execz (the tick writer: one thread of the launch) is skipped, every later s_cbranch_execz region is entered (a finished
sub-lane exists), and an s_cbranch_execnz in a block that did not touch exec is taken (a running wave has a lane)."""
import heapq
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HEADLINE = "step_kernel<CartPole,4,true,false,15,1>"
VALU_BEFORE_BY_HAND = 428
VALU_NOW = 394
SADDR_LOAD = re.compile(r"global_load_dwordx4 v\[\d+:\d+\], v\d+, s\[\d+:\d+\]")
SADDR_STORE = re.compile(r"global_store_dword(x4)? v\d+, v(\d+|\[\d+:\d+\]), s\[\d+:\d+\]")


def _blocks(lines):
    """Basic blocks of one function: [{"labels", "ins", "succ"}], block 0 the main entry."""
    if any(l.startswith("s_branch") for l in lines[:8]):                 # the compatibility prologue ends with a branch to the main entry
        lines = lines[next(i for i, l in enumerate(lines) if l.startswith("s_branch")) + 1:]
    blocks, cur = [], {"labels": [], "ins": []}
    for l in lines:
        l = l.split(";")[0].strip()
        if not l:
            continue
        if l.endswith(":"):
            if cur["ins"]:
                blocks.append(cur)
                cur = {"labels": [], "ins": []}
            cur["labels"].append(l[:-1])
            continue
        if l.startswith("."):
            continue
        cur["ins"].append(l)
        if l.startswith(("s_branch", "s_cbranch", "s_endpgm")):
            blocks.append(cur)
            cur = {"labels": [], "ins": []}
    if cur["ins"]:
        blocks.append(cur)
    at = {x: i for i, b in enumerate(blocks) for x in b["labels"]}
    seen_load = False
    for i, b in enumerate(blocks):
        seen_load = seen_load or any(l.startswith("global_load") for l in b["ins"])
        last = b["ins"][-1]
        m = re.match(r"s_c?branch\w*\s+(\S+)", last)
        if last.startswith("s_endpgm"):
            b["succ"] = []
        elif last.startswith("s_branch"):
            b["succ"] = [at[m.group(1)]]
        elif last.startswith("s_cbranch_execnz") and not any("exec" in l for l in b["ins"][:-1]):
            b["succ"] = [at[m.group(1)]]
        elif last.startswith("s_cbranch_execz"):
            b["succ"] = [i + 1] if seen_load else [at[m.group(1)]]
        elif last.startswith("s_cbranch"):
            b["succ"] = [at[m.group(1)], i + 1]
        else:
            b["succ"] = [i + 1] if i + 1 < len(blocks) else []
    return blocks


def _valu(ins):
    return sum(1 for l in ins if l.startswith("v_"))


def _cheapest(blocks, src, dst, weight):
    """(VALU count, block path) of the cheapest route src -> dst, both ends included"""
    best, prev, heap = {src: weight(src)}, {}, [(weight(src), src)]
    while heap:
        c, i = heapq.heappop(heap)
        if c > best[i]:
            continue
        if i == dst:
            path = [dst]
            while path[-1] != src:
                path.append(prev[path[-1]])
            return c, path[::-1]
        for j in blocks[i]["succ"]:
            if c + weight(j) < best.get(j, 1 << 30):
                best[j], prev[j] = c + weight(j), i
                heapq.heappush(heap, (best[j], j))
    return None


def route(lines):
    """(VALU count, instructions) of the full-workgroup, small-angle, single-trip route up to its last store."""
    blocks = _blocks(lines)
    ends = [i for i, b in enumerate(blocks) if sum(1 for l in b["ins"] if SADDR_STORE.match(l) and "dwordx4" in l) >= 4]
    assert len(ends) == 1, "one block stores the four state rows of the unguarded body with scalar bases: %r" % ends
    end = ends[0]
    cut = max(k for k, l in enumerate(blocks[end]["ins"]) if l.startswith("global_store")) + 1

    def weight(i):
        return _valu(blocks[i]["ins"][:cut]) if i == end else _valu(blocks[i]["ins"])

    found = None
    for x, b in enumerate(blocks):
        if not any(l.startswith("ds_write_b128") for l in b["ins"]):
            continue
        head, tail = _cheapest(blocks, 0, x, weight), _cheapest(blocks, x, end, weight)
        if head and tail and (found is None or head[0] + tail[0] - weight(x) < found[0]):
            found = (head[0] + tail[0] - weight(x), head[1] + tail[1][1:])
    assert found, "no route from the entry through a reset draw to the state stores"
    ins = []
    for i in found[1]:
        ins += blocks[i]["ins"][:cut] if i == end else blocks[i]["ins"]
    return found[0], ins


def _function_lines(path, name):
    """The instruction lines of kernel `name` (as tools/kernel_resources.py prints it), out-of-line blocks behind its s_endpgm included."""
    text = open(path).read()
    mangled = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
    dem = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True).stdout.split("\n")
    for m, d in zip(mangled, dem):
        if re.sub(r"\(.*\)$", "", d.replace("gymnet::", "").replace("void ", "")).replace(", ", ",") == name:
            start = text.index("\n" + m + ":")
            body = text[start:text.index(".Lfunc_end", start)]
            return [l.strip() for l in body.split("\n")[2:]]
    raise AssertionError("no kernel " + name)


@pytest.fixture(scope="module")
def headline():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    import kernel_resources
    with tempfile.TemporaryDirectory() as d:
        path = kernel_resources.assembly("cartpole", d)
        lines = _function_lines(path, HEADLINE)
        res = kernel_resources.kernels(path)[HEADLINE]
    return lines, res


@pytest.mark.timeout(900)
def test_loads_and_stores_of_the_full_workgroup_route_use_scalar_bases(headline):
    _, ins = route(headline[0])
    loads = [l for l in ins if l.startswith("global_load")]
    stores = [l for l in ins if l.startswith("global_store")]
    assert len(loads) == 5 and all(SADDR_LOAD.match(l) for l in loads), loads
    assert len(stores) == 6 and all(SADDR_STORE.match(l) for l in stores), stores
    assert not [l for l in ins if l.startswith(("flat_", "scratch_", "buffer_"))]


@pytest.mark.timeout(900)
def test_headline_kernel_keeps_eight_waves_per_simd(headline):
    res = headline[1]
    assert res["vgpr"] <= 64 and res["scratch"] == 0 and res["occupancy"] == 8, res


@pytest.mark.timeout(900)
def test_valu_count_of_the_full_workgroup_route(headline):
    count, ins = route(headline[0])
    print("VALU on the full-workgroup, small-angle, single-trip route:", count)
    assert any(l.startswith("ds_read_b128") for l in ins)                # the reset's hand-back is on the route
    assert count < VALU_BEFORE_BY_HAND
    assert count <= VALU_NOW, count
