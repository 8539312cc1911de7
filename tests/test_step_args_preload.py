"""The one-step kernels take their first-use argument words as flat leading arguments so that gfx950 delivers them in user SGPRs at wave
launch (csrc/kernels.hpp StepKernelFn, -mllvm -amdgpu-kernarg-preload-count=14 in the product's flags).  Asserted from the assembly the
product's flags produce (tools/kernel_resources.py FLAGS; no GPU, about a minute of hipcc):
  * every step_kernel / step_kernel_pipe / step_kernel_pipe2 instantiation of cartpole, cartpole64, acrobot and mountaincar has the
    preload length the probe kernels had (14 dwords: profiles/launch_floor.txt, tests/test_launch_floor_probe.py);
  * in the headline kernel no wave waits for a scalar load before its first vector load.  The instructions are followed the way every
    wave but ONE runs them: the block that writes the next tick (thread 0 of workgroup 0, behind an s_cbranch_execz) is skipped.
The set of kernel names is pinned by tests/test_instantiation_coverage.py."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ENVS = ("cartpole", "cartpole64", "acrobot", "mountaincar")
PRELOAD_DWORDS = 14
HEADLINE = "step_kernel<CartPole,4,true,false,15,1>"


def _parse(path):
    """{kernel name as kernel_resources prints it: (preload length, instruction lines of the function)}"""
    text = open(path).read()
    mangled = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
    dem = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for m, d in zip(mangled, dem):
        name = re.sub(r"\(.*\)$", "", d.replace("gymnet::", "").replace("void ", "")).replace(", ", ",")
        desc = text[text.index(".amdhsa_kernel " + m):]
        desc = desc[:desc.index(".end_amdhsa_kernel")]
        length = int(re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", desc).group(1))
        start = text.index("\n" + m + ":")
        body = text[start:text.index("s_endpgm", start)]
        out[name] = (length, [l.strip() for l in body.split("\n")[2:]])
    return out


@pytest.fixture(scope="module")
def step_kernels():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    import kernel_resources
    assert "-amdgpu-kernarg-preload-count=%d" % PRELOAD_DWORDS in kernel_resources.FLAGS      # "the product's flags"
    with tempfile.TemporaryDirectory() as d:
        with ThreadPoolExecutor(max_workers=len(ENVS)) as ex:
            paths = list(ex.map(lambda e: kernel_resources.assembly(e, d), ENVS))
        k = {}
        for p in paths:
            k.update(_parse(p))
    return {n: v for n, v in k.items() if n.startswith(("step_kernel<", "step_kernel_pipe<", "step_kernel_pipe2<"))}


@pytest.mark.timeout(900)
def test_every_one_step_kernel_preloads_its_first_use_words(step_kernels):
    assert HEADLINE in step_kernels and len(step_kernels) > 50
    bad = {n: v[0] for n, v in step_kernels.items() if v[0] != PRELOAD_DWORDS}
    assert not bad, bad


def _until_first_vector_load(lines):
    """The instructions a wave WITHOUT thread 0 of workgroup 0 runs from the main entry to its first global_load."""
    if any(l.startswith("s_branch") for l in lines[:8]):                 # the compatibility prologue ends with a branch to the main entry
        lines = lines[next(i for i, l in enumerate(lines) if l.startswith("s_branch")) + 1:]
    seen, skip_to = [], None
    for l in lines:
        if skip_to is not None:
            if l.startswith(skip_to + ":"):
                skip_to = None
            continue
        if not l or l.startswith((";", ".")) or l.endswith(":"):
            continue
        seen.append(l)
        if l.startswith("global_load"):
            return seen
        m = re.match(r"s_cbranch_execz\s+(\S+)", l)
        if m:
            skip_to = m.group(1)
    raise AssertionError("no global_load found")


@pytest.mark.timeout(900)
def test_headline_kernel_issues_its_first_vector_load_without_waiting_for_a_scalar_load(step_kernels):
    head = _until_first_vector_load(step_kernels[HEADLINE][1])
    waits = [l for l in head if l.startswith("s_waitcnt") and "lgkmcnt" in l]
    assert not waits, head
