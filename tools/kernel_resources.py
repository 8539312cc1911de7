#!/usr/bin/env python3
"""Register / LDS / scratch budget of every kernel instantiation, read from the gfx950 assembly the product's flags produce (no GPU needed):
VGPRs -> waves per SIMD (512 / VGPRs, at most 8), scratch bytes (spills), static LDS bytes.  Round 5 found two slowdowns that only this view
explains — a float32 bookkeeping rollout that allocated 131-152 VGPRs (three waves per SIMD where 2^20 lanes need four) and a float64
four-pair kernel that must stay at two waves per SIMD because it spills when capped for three (profiles/occupancy_hints_r05.txt).
    python tools/kernel_resources.py [env ...]        env: the env_<env>.hip units of gym.net_amd/build.py's SOURCES (default: all),
                                                      or any unit of SOURCES by file name (action_repeat.hip)
Prints one line per kernel; tests/test_kernel_resources.py asserts the invariants the launch policy relies on."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym.net_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def _product_build():
    """gym.net_amd/build.py: the one place that names the translation units and the product's flags"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_gymnet_build", os.path.join(ROOT, "gym.net_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_BUILD = _product_build()
FLAGS = [f for f in _BUILD.FLAGS if f not in ("-fPIC", "-shared")] + ["--cuda-device-only", "-S"]
# every env unit of the product (build.py SOURCES), in the command line's default ...
CLI_ENVS = tuple(s[len("env_"):-len(".hip")] for s in _BUILD.SOURCES if s.startswith("env_"))
# ... while collect()'s default stays the five units tests/_instantiation_matrix.py covers; the newer units have their own recipe tables
# (tests/_mountaincar_continuous_matrix.py)
ENVS = tuple(e for e in CLI_ENVS if e != "mountaincar_continuous")


def assembly(env, outdir):
    unit = env if env.endswith(".hip") else f"env_{env}.hip"
    out = os.path.join(outdir, os.path.splitext(unit)[0] + ".s")
    r = subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, unit), "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    return out


def kernels(path):
    """{demangled kernel name without parameter list: {"vgpr", "occupancy", "scratch", "lds"}}"""
    lines = open(path).read().split("\n")
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l)]
    names = [lines[i].split(":")[0] for i in starts]
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for idx, i in enumerate(starts):
        j = starts[idx + 1] if idx + 1 < len(starts) else len(lines)
        meta = {}
        for l in lines[i:j]:
            m = re.match(r";\s*(NumVgprs|ScratchSize|Occupancy|LDSByteSize):\s*(\d+)", l.strip())
            if m:
                meta[m.group(1)] = int(m.group(2))
        if "NumVgprs" not in meta:
            continue
        name = re.sub(r"\(.*\)$", "", dem[idx].replace("(anonymous namespace)::", "").replace("gymnet::", "").replace("void ", "")).replace(", ", ",")
        out[name] = {"vgpr": meta["NumVgprs"], "occupancy": meta.get("Occupancy", -1), "scratch": meta.get("ScratchSize", 0), "lds": meta.get("LDSByteSize", 0)}
    return out


def collect(envs=ENVS):
    with tempfile.TemporaryDirectory() as d:
        with ThreadPoolExecutor(max_workers=min(len(envs), os.cpu_count() or 4)) as ex:
            paths = list(ex.map(lambda e: assembly(e, d), envs))
        res = {}
        for p in paths:
            res.update(kernels(p))
    return res


if __name__ == "__main__":
    envs = tuple(sys.argv[1:]) or CLI_ENVS
    res = collect(envs)
    units = " ".join(e if e.endswith(".hip") else f"env_{e}.hip" for e in envs)
    print(f"# hipcc {' '.join(FLAGS)}  (gym.net_amd/csrc/: {units})   waves per SIMD = min(8, 512 // VGPRs)")
    print(f"{'kernel':72s} {'VGPRs':>6s} {'waves/SIMD':>10s} {'scratch B':>10s} {'LDS B':>7s}")
    for k in sorted(res):
        v = res[k]
        print(f"{k:72s} {v['vgpr']:6d} {v['occupancy']:10d} {v['scratch']:10d} {v['lds']:7d}")
