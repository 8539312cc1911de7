"""Times gymnet_rollout_inputs_device (gym.net_amd/csrc/rollout_inputs.hip) with HIP events in one process, beside a device-to-device
hipMemcpyAsync of the same output bytes (the floor of a write-bound call) and the torch loop the actor probes use to rebuild the inputs
(tools/actor_logp_probe.py, torch_c's history part without the network: a Python loop over T that shifts an [n, S, obs_dim] tensor with
torch.where).

    python tools/rollout_inputs_probe.py [--build-only] [--reps 10] [--passes 2] [--out profiles/rollout_inputs_probe.txt]

CartPole's shape, obs_dim 4 at S = 4 (rows of 16 floats), random observations, a done rate of 0.02.
Dense:    2^20 lanes x T = 16 and 2^16 lanes x T = 256: 81 B per row (17 read: 4 floats and a done byte; 64 written), 1.07 GB written.
Gathered: records of 2^20 lanes x T = 256, 2^16 random rows; the torch side is the same loop followed by an index.
Candidates: the product's kernels, and rollout_inputs.hip rebuilt (small libraries under tools/build/, built by --build-only or on first
use, each linked against the product library for its error helpers) with
  -DGYMNET_ROLLOUT_INPUTS_LANE_MAJOR=1        neighbouring threads own neighbouring lanes: a wave's store instruction writes 16 bytes at
                                              a stride of one row (64 B), the pattern of a thread that owns a whole lane's row
  -DGYMNET_ROLLOUT_INPUTS_TARGET_THREADS=0    one chunk: every thread walks all T rows
  -DGYMNET_ROLLOUT_INPUTS_TARGET_THREADS=...  a quarter of the product's target: a quarter of the chunks
and the product's kernel at one float per thread (d_x one float off its 16-byte boundary).  Every candidate's output is compared with the
product kernel's, bit for bit, and so is the torch loop's (started from the same history).  Per row: median us of --reps timings (min ..
max), GB/s over the bytes moved and the share of the 8 TB/s HBM peak.  The candidates alternate, and the whole measurement runs --passes
times so that the spread shows.  Needs a GPU; no fallback."""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BUILD_DIR = os.path.join(ROOT, "tools", "build")
TARGET = 32 * 64 * 1024
VARIANTS = {"lane-major": ["-DGYMNET_ROLLOUT_INPUTS_LANE_MAJOR=1"], "one chunk": ["-DGYMNET_ROLLOUT_INPUTS_TARGET_THREADS=0"],
            "a quarter of the chunks": [f"-DGYMNET_ROLLOUT_INPUTS_TARGET_THREADS={TARGET // 4}"]}
DENSE = [(1 << 20, 16), (1 << 16, 256)]
GATHER = (1 << 20, 256, 1 << 16)
O, S = 4, 4
W = O * S
PEAK_GBS = 8000.0
CHUNK = 16                                   # tools/actor_logp_probe.py


def variant_path(name):
    return os.path.join(BUILD_DIR, "librollout_inputs_" + name.replace(" ", "_").replace("-", "_") + ".so")


def build_variants(pkg_lib, force=False):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    build = kernel_resources._BUILD
    os.makedirs(BUILD_DIR, exist_ok=True)
    lib_dir = os.path.dirname(pkg_lib)
    for name, defines in VARIANTS.items():
        out = variant_path(name)
        if os.path.exists(out) and not force:
            continue
        cmd = [build.hipcc()] + build.FLAGS + defines + [os.path.join(build.CSRC, "rollout_inputs.hip"), "-L", lib_dir, "-lgymnet_amd",
                                                         "-Wl,-rpath,$ORIGIN/../../gym.net_amd/lib", "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("rollout_inputs_probe: hipcc failed:\n" + " ".join(cmd) + "\n" + r.stderr[-3000:])
        print("built", os.path.relpath(out, ROOT), flush=True)


def prototype(lib):
    P, I64, I32 = C.c_void_p, C.c_int64, C.c_int32
    lib.gymnet_rollout_inputs_device.restype = C.c_int
    lib.gymnet_rollout_inputs_device.argtypes = [C.c_int, P, I64, I64, I64, I32, I32, I32, P, P, P, I64, P, I64, P, I64, P, I64]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    build_variants(pkg.LIB_PATH, force=args.build_only)
    if args.build_only:
        return
    import torch
    if pkg.device_count() < 1:
        raise SystemExit("rollout_inputs_probe: no GPU")
    product = prototype(C.CDLL(pkg.LIB_PATH))
    variants = {name: prototype(C.CDLL(variant_path(name))) for name in VARIANTS}
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def inputs(lib, T, n, obs, done, h0, x, rows=None, hout=None):
        st = lib.gymnet_rollout_inputs_device(0, None, T, n, n, O, S, 0, ptr(obs), ptr(done), ptr(h0), n, ptr(rows), 0 if rows is None else rows.numel(),
                                              ptr(x), W, ptr(hout), n)
        if st != 0:
            raise SystemExit(f"rollout_inputs_probe: gymnet_rollout_inputs_device returned {st}")

    def memcpy(dst, src):
        if hip.hipMemcpyAsync(ptr(dst), ptr(src), dst.numel() * 4, 3, None) != 0:          # hipMemcpyDeviceToDevice, the default stream
            raise SystemExit("rollout_inputs_probe: hipMemcpyAsync failed")

    def torch_loop(T, n, rec_obs, rec_done, h0, hist, x):
        """tools/actor_logp_probe.py's rebuild, the network left out; started from the history the rollout started from, so that it is exact"""
        with torch.no_grad():
            hist.copy_(h0.permute(2, 0, 1))
            for t0 in range(0, T, CHUNK):
                xs = []
                for t in range(t0, min(T, t0 + CHUNK)):
                    xs.append(hist.reshape(n, S * O).clone())
                    o = rec_obs[t].t()
                    rolled = torch.cat([hist[:, 1:], o[:, None, :]], dim=1)
                    hist.copy_(torch.where((rec_done[t] != 0)[:, None, None], o[:, None, :].expand(n, S, O), rolled))
                x[t0:t0 + len(xs)] = torch.stack(xs)

    def timed(fn, reps):
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return float(np.median(ts)), float(min(ts)), float(max(ts))

    lines = [f"gymnet_rollout_inputs_device, obs_dim {O}, history {S} (rows of {W} floats), float32, done rate 0.02, HIP events on the default stream, "
             f"median of {args.reps} (min .. max) us; GB/s over the bytes moved; share of {PEAK_GBS / 1000:.0f} TB/s",
             f"device: {torch.cuda.get_device_name(0)}"]

    def row(label, us, lo, hi, nbytes, extra=""):
        gbs = nbytes / us / 1e3
        line = f"  {label:38s} {us:10.1f} us ({lo:9.1f} .. {hi:9.1f})  {gbs:8.1f} GB/s  {100 * gbs / PEAK_GBS:5.1f} % of peak{extra}"
        print(line, flush=True)
        lines.append(line)

    def records(T, n):
        gen = torch.Generator(device="cuda").manual_seed(1)
        obs = torch.randn((T, O, n), device="cuda", generator=gen)
        done = (torch.rand((T, n), device="cuda", generator=gen) < 0.02).to(torch.uint8)
        h0 = torch.randn((S, O, n), device="cuda", generator=gen)
        return obs, done, h0

    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    loop_reps = max(3, args.reps // 3)
    for n, T in DENSE:
        obs, done, h0 = records(T, n)
        x, ref, src = (torch.empty((T, n, W), device="cuda") for _ in range(3))
        x1 = torch.empty(T * n * W + 1, device="cuda")[1:].view(T, n, W)       # one float off the 16-byte boundary: one float per thread
        hist = torch.empty((n, S, O), device="cuda")
        src.normal_()
        torch.cuda.synchronize()
        inputs(product, T, n, obs, done, h0, ref)
        moved, written = T * n * (O * 4 + 1 + W * 4), T * n * W * 4
        head = f"dense, lanes {n} (2^{n.bit_length() - 1}) x T = {T}: {written / 1e9:.2f} GB written, {moved / 1e9:.2f} GB moved"
        print(head, flush=True)
        lines.append(head)
        for name, lib in variants.items():                                      # every candidate computes the product kernel's bits
            x.fill_(-7.0)
            inputs(lib, T, n, obs, done, h0, x)
            torch.cuda.synchronize()
            if not same(x, ref):
                raise SystemExit(f"rollout_inputs_probe: candidate {name!r} differs from the product kernel")
        inputs(product, T, n, obs, done, h0, x1)
        torch_loop(T, n, obs, done, h0, hist, x)
        torch.cuda.synchronize()
        if not (same(x, ref) and same(x1, ref)):
            raise SystemExit("rollout_inputs_probe: the torch loop or the one-float form differs from the product kernel")
        lines.append("  every candidate, the one-float form and the torch loop give the product kernel's bits")
        print(lines[-1], flush=True)
        for p in range(args.passes):
            lines.append(f" pass {p + 1}")
            print(lines[-1], flush=True)
            kernel = lambda: inputs(product, T, n, obs, done, h0, x)
            copy = lambda: memcpy(x, src)
            loop = lambda: torch_loop(T, n, obs, done, h0, hist, x)
            for fn in (kernel, copy, loop):
                fn()                                                            # warm
            torch.cuda.synchronize()
            for again in ("", " (again)"):                                      # alternating
                k_us, k_lo, k_hi = timed(kernel, args.reps)
                row("product kernel" + again, k_us, k_lo, k_hi, moved)
                c_us, c_lo, c_hi = timed(copy, args.reps)
                row("hipMemcpyAsync of the output" + again, c_us, c_lo, c_hi, 2 * written, f"  kernel = {k_us / c_us:.2f} x the copy")
                t_us, t_lo, t_hi = timed(loop, loop_reps)
                row("torch loop" + again, t_us, t_lo, t_hi, moved, f"  = {t_us / k_us:.1f} x the kernel")
            for name, lib in variants.items():
                fn = lambda: inputs(lib, T, n, obs, done, h0, x)
                fn()
                torch.cuda.synchronize()
                row(name, *timed(fn, args.reps), moved)
            fn = lambda: inputs(product, T, n, obs, done, h0, x1)
            fn()
            torch.cuda.synchronize()
            row("one float per thread", *timed(fn, args.reps), moved)
            row("product kernel (last)", *timed(kernel, args.reps), moved)
        del obs, done, h0, x, ref, src, x1, hist
        torch.cuda.empty_cache()
    n, T, m = GATHER
    obs, done, h0 = records(T, n)
    rows = torch.randint(0, T * n, (m,), device="cuda", dtype=torch.int64, generator=torch.Generator(device="cuda").manual_seed(2))
    x, ref = torch.empty((m, W), device="cuda"), torch.empty((m, W), device="cuda")
    dense = torch.empty((T, n, W), device="cuda")                               # what the torch side has to materialise: 17 GB
    hist = torch.empty((n, S, O), device="cuda")
    torch.cuda.synchronize()
    moved = m * (O * 4 * S + (S - 1) + 8 + W * 4)                               # per row at most: S observations, S - 1 done bytes, the index, the row
    head = f"gathered, records of lanes {n} (2^{n.bit_length() - 1}) x T = {T}, {m} (2^{m.bit_length() - 1}) random rows: {m * W * 4 / 1e6:.1f} MB written"
    print(head, flush=True)
    lines.append(head)
    inputs(product, T, n, obs, done, h0, ref, rows=rows)

    def loop_and_index():
        torch_loop(T, n, obs, done, h0, hist, dense)
        x.copy_(dense.view(T * n, W)[rows])
    loop_and_index()
    torch.cuda.synchronize()
    if not same(x, ref):
        raise SystemExit("rollout_inputs_probe: the torch loop and index differ from the gathered kernel")
    for name, lib in variants.items():
        x.fill_(-7.0)
        inputs(lib, T, n, obs, done, h0, x, rows=rows)
        torch.cuda.synchronize()
        if not same(x, ref):
            raise SystemExit(f"rollout_inputs_probe: candidate {name!r} differs from the gathered kernel")
    lines.append("  the torch loop followed by an index and every candidate give the gathered kernel's bits")
    print(lines[-1], flush=True)
    for p in range(args.passes):
        lines.append(f" pass {p + 1}")
        print(lines[-1], flush=True)
        kernel = lambda: inputs(product, T, n, obs, done, h0, x, rows=rows)
        kernel()
        torch.cuda.synchronize()
        for again in ("", " (again)"):
            k_us, k_lo, k_hi = timed(kernel, args.reps)
            row("gathered kernel" + again, k_us, k_lo, k_hi, moved)
            t_us, t_lo, t_hi = timed(loop_and_index, 2)
            row("torch loop + index" + again, t_us, t_lo, t_hi, moved, f"  = {t_us / k_us:.0f} x the kernel")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
