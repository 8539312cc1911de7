"""tools/launch_floor_probe.hip measures what the kernel-argument scalar loads cost on the launch floor (profiles/launch_floor.txt,
docs/ledger.md §16: a quarter of a microsecond per round trip at 2^20 lanes, which only variant (e) collects — the form the step kernels took).  What the measurement means rests on what the
compiler made of each variant, so that is asserted here from the gfx950 assembly (no GPU, a few seconds of hipcc):
  * the by-value struct is never preloaded, the flat arguments are only under the flag, and 14 dwords is the ceiling;
  * variant (c), the flat signature with the flag, STILL waits for a scalar load before its first vector load (the workgroup size is a
    hidden kernel argument and the tick's parity sits in the trailing struct), while variant (e) does not."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
BASE = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "--cuda-device-only", "-S"]
PRELOAD = ["-mllvm", "-amdgpu-kernarg-preload-count=14", "-DLAUNCH_FLOOR_PRELOAD_UNIT"]


def _kernels(path):
    """{kernel name: (preload length, instructions of the main entry up to and including the first global_load)}"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z(\d+)(floor_\w+)):.*?\n(.*?)s_endpgm", text, re.S | re.M):
        mangled, name, body = m.group(1), m.group(3)[:int(m.group(2))], m.group(4)
        desc = text[text.index(".amdhsa_kernel " + mangled):]
        length = int(re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", desc).group(1))
        # past the compatibility prologue (it ends with a branch to the 256-byte aligned main entry)
        if "s_branch" in body:
            body = body[body.index("s_branch"):]
        head = []
        for line in body.split("\n"):
            ins = line.strip().split(" ")[0].split("\t")[0]
            if not ins or ins.startswith((";", ".")):
                continue
            head.append(line.strip())
            if ins.startswith("global_load"):
                break
        out[name] = (length, head)
    return out


@pytest.fixture(scope="module")
def probe_kernels():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "tools", "launch_floor_probe.hip")
    with tempfile.TemporaryDirectory() as d:
        jobs = [(os.path.join(d, "main.s"), []), (os.path.join(d, "preload.s"), PRELOAD)]
        procs = [subprocess.Popen([HIPCC] + BASE + extra + [src, "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                 for out, extra in jobs]
        for p in procs:
            log = p.communicate()[0]
            assert p.returncode == 0, log[-1500:]
        k = {}
        for out, _ in jobs:
            k.update(_kernels(out))
    return k


def test_only_flat_arguments_under_the_flag_are_preloaded(probe_kernels):
    lengths = {name: v[0] for name, v in probe_kernels.items()}
    assert lengths == {"floor_empty": 0, "floor_struct": 0, "floor_flat": 0, "floor_flat_preload": 14, "floor_flat_preload_all": 14}


def _waits_before_first_load(head):
    assert head and head[-1].startswith("global_load"), head
    return any(l.startswith("s_waitcnt") and "lgkmcnt" in l for l in head[:-1])


def test_which_variants_wait_for_a_scalar_load_before_the_first_vector_load(probe_kernels):
    assert _waits_before_first_load(probe_kernels["floor_struct"][1])
    assert _waits_before_first_load(probe_kernels["floor_flat"][1])
    # the flat signature with the flag: the workgroup size (hidden argument) is still loaded and waited for
    head_c = probe_kernels["floor_flat_preload"][1]
    assert _waits_before_first_load(head_c) and any(l.startswith("s_load") for l in head_c), head_c
    # workgroup size and parity as flat words: nothing is loaded before the first vector load
    head_e = probe_kernels["floor_flat_preload_all"][1]
    assert not _waits_before_first_load(head_e) and not any(l.startswith("s_load") for l in head_e), head_e
