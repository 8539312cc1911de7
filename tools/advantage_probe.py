"""Times gymnet_gae_device (gym.net_amd/csrc/advantage.hip) with HIP events in one process, beside the torch loop a user would otherwise
write: a backward loop over T of elementwise launches with torch.where.

    python tools/advantage_probe.py [--build-only] [--reps 10] [--passes 2] [--out profiles/advantage_probe.txt]

Shapes: 2^20 lanes x T = 256 (the README's) and 2^14 lanes x T = 2048 (few threads, long chains).
Forms:  gae        values, last value, both outputs, out of place          17 B per lane-step
        gae-inplace  advantage over reward, return over value              17 B
        lean       no values, advantage only (the reward-to-go)             9 B
Candidates: the product's kernel (its own V, U and cache hint per lane count: advantage.hpp / advantage.hip), and advantage.hip rebuilt
with every U in {2, 4, 8} (rows in flight) x {plain, non-temporal} accesses and no small-batch threshold (-DGYMNET_ADVANTAGE_U /
-DGYMNET_ADVANTAGE_NT / -DGYMNET_ADVANTAGE_NARROW_BELOW=0; small libraries under tools/build/, built by --build-only or on first use,
each linked against the product library for its error helpers), at V = 4 and, with the advantage array one element off its 16-byte
boundary, at V = 1; then V = 4 against V = 1 over lane counts from 2^10 to 2^20 at T = 256.  Every candidate's output is compared with the product kernel's, bit for bit, at the
timed shape.  Per row: median us of --reps timings, GB/s over the bytes the form moves (computed here from the shapes) and the share of
the 8 TB/s HBM peak.  The kernel and the torch loop alternate, and the whole measurement runs --passes times so that the spread shows.
Needs a GPU; no fallback."""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BUILD_DIR = os.path.join(ROOT, "tools", "build")
VARIANTS = [(u, nt) for u in (2, 4, 8) for nt in (0, 3)] + [(4, 1), (4, 2)]        # nt: bit 0 non-temporal loads, bit 1 stores
HINT = {0: 'plain', 1: 'nt loads', 2: 'nt stores', 3: 'non-temporal'}
SHAPES = [(1 << 20, 256), (1 << 14, 2048)]
PEAK_GBS = 8000.0
GAMMA, LAM = 0.99, 0.95
BYTES = {"gae": 17, "gae-inplace": 17, "lean": 9}


def variant_path(u, nt):
    return os.path.join(BUILD_DIR, f"libadvantage_u{u}_nt{nt}.so")


def build_variants(pkg_lib, force=False):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    build = kernel_resources._BUILD
    os.makedirs(BUILD_DIR, exist_ok=True)
    lib_dir = os.path.dirname(pkg_lib)
    for u, nt in VARIANTS:
        out = variant_path(u, nt)
        if os.path.exists(out) and not force:
            continue
        cmd = [build.hipcc()] + build.FLAGS + [f"-DGYMNET_ADVANTAGE_U={u}", f"-DGYMNET_ADVANTAGE_NT={nt}", "-DGYMNET_ADVANTAGE_NARROW_BELOW=0", os.path.join(build.CSRC, "advantage.hip"),
                                              "-L", lib_dir, "-lgymnet_amd", "-Wl,-rpath,$ORIGIN/../../gym.net_amd/lib", "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("advantage_probe: hipcc failed:\n" + " ".join(cmd) + "\n" + r.stderr[-3000:])
        print("built", os.path.relpath(out, ROOT), flush=True)


def prototype(lib):
    P = C.c_void_p
    lib.gymnet_gae_device.restype = C.c_int
    lib.gymnet_gae_device.argtypes = [C.c_int, P, C.c_int64, C.c_int64, C.c_int64, P, P, P, P, P, C.c_float, C.c_float, P, P]
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
        raise SystemExit("advantage_probe: no GPU")
    product = prototype(C.CDLL(pkg.LIB_PATH))
    variants = {v: prototype(C.CDLL(variant_path(*v))) for v in VARIANTS}
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def gae(lib, T, n, r, d, v, vlast, adv, ret):
        st = lib.gymnet_gae_device(0, None, T, n, n, ptr(r), ptr(d), ptr(v), ptr(vlast), None, GAMMA, LAM, ptr(adv), ptr(ret))
        if st != 0:
            raise SystemExit(f"advantage_probe: gymnet_gae_device returned {st}")

    def torch_loop(T, r, d, v, vlast, adv, ret):
        """the loop the README would otherwise tell a user to write (no boot: a truncation counts as a termination)"""
        A = torch.zeros_like(vlast)
        vnext = vlast
        gl = GAMMA * LAM
        for t in range(T - 1, -1, -1):
            cut = d[t] != 0
            delta = r[t] + GAMMA * torch.where(cut, 0.0, vnext) - v[t]
            A = torch.where(cut, delta, delta + gl * A)
            adv[t] = A
            ret[t] = A + v[t]
            vnext = v[t]

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

    lines = [f"gymnet_gae_device, gamma {GAMMA} lambda {LAM}, float32, done rate 0.02 (bytes 1 / 2), HIP events on the default stream, "
             f"median of {args.reps} (min .. max) us; GB/s over the form's bytes; share of {PEAK_GBS / 1000:.0f} TB/s",
             f"device: {torch.cuda.get_device_name(0)}"]

    def row(label, us, lo, hi, nbytes, extra=""):
        gbs = nbytes / us / 1e3
        line = f"  {label:34s} {us:10.1f} us ({lo:9.1f} .. {hi:9.1f})  {gbs:8.1f} GB/s  {100 * gbs / PEAK_GBS:5.1f} % of peak{extra}"
        print(line, flush=True)
        lines.append(line)

    for n, T in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(1)
        r0 = torch.randn((T, n), device="cuda", generator=gen)
        v0 = torch.randn((T, n), device="cuda", generator=gen)
        vlast = torch.randn((n,), device="cuda", generator=gen)
        u = torch.rand((T, n), device="cuda", generator=gen)
        d = torch.where(u < 0.01, 1, torch.where(u < 0.02, 2, 0)).to(torch.uint8)
        del u
        adv, ret, adv_ref, ret_ref = (torch.empty((T, n), device="cuda") for _ in range(4))
        r_ip, v_ip = torch.empty_like(r0), torch.empty_like(v0)
        torch.cuda.synchronize()
        gae(product, T, n, r0, d, v0, vlast, adv_ref, ret_ref)
        torch.cuda.synchronize()
        head = f"lanes {n} (2^{n.bit_length() - 1}) x T = {T}: {T * n * 17 / 1e9:.2f} GB (gae), {T * n * 9 / 1e9:.2f} GB (lean)"
        print(head, flush=True)
        lines.append(head)
        # every candidate computes the product kernel's bits
        for key, lib in variants.items():
            adv.fill_(-7.0); ret.fill_(-7.0)
            gae(lib, T, n, r0, d, v0, vlast, adv, ret)
            torch.cuda.synchronize()
            if not (torch.equal(adv.view(torch.int32), adv_ref.view(torch.int32)) and torch.equal(ret.view(torch.int32), ret_ref.view(torch.int32))):
                raise SystemExit(f"advantage_probe: candidate U={key[0]} NT={key[1]} differs from the product kernel")
        # ... and the torch loop agrees with it to rounding (it fuses nothing and sums in another order: not bit for bit)
        torch_loop(T, r0, d, v0, vlast, adv, ret)
        torch.cuda.synchronize()
        dev = float((adv - adv_ref).abs().max())
        lines.append(f"  torch loop against the kernel: worst |difference| {dev:.2e}")
        print(lines[-1], flush=True)
        tot = T * n
        loop_reps = max(3, args.reps // 3)
        for p in range(args.passes):
            lines.append(f" pass {p + 1}")
            print(lines[-1], flush=True)
            for fn in (lambda: gae(product, T, n, r0, d, v0, vlast, adv, ret), lambda: torch_loop(T, r0, d, v0, vlast, adv, ret)):
                fn()                                                    # warm
            torch.cuda.synchronize()
            k_us, k_lo, k_hi = timed(lambda: gae(product, T, n, r0, d, v0, vlast, adv, ret), args.reps)
            t_us, t_lo, t_hi = timed(lambda: torch_loop(T, r0, d, v0, vlast, adv, ret), loop_reps)
            k2_us, k2_lo, k2_hi = timed(lambda: gae(product, T, n, r0, d, v0, vlast, adv, ret), args.reps)
            t2_us, t2_lo, t2_hi = timed(lambda: torch_loop(T, r0, d, v0, vlast, adv, ret), loop_reps)
            row("gae, product kernel", k_us, k_lo, k_hi, tot * BYTES["gae"])
            row("gae, torch loop", t_us, t_lo, t_hi, tot * BYTES["gae"], f"  = {t_us / k_us:.1f} x the kernel")
            row("gae, product kernel (again)", k2_us, k2_lo, k2_hi, tot * BYTES["gae"])
            row("gae, torch loop (again)", t2_us, t2_lo, t2_hi, tot * BYTES["gae"], f"  = {t2_us / k2_us:.1f} x the kernel")

            def in_place():
                gae(product, T, n, r_ip, d, v_ip, vlast, r_ip, v_ip)
            r_ip.copy_(r0); v_ip.copy_(v0)
            in_place()                                                  # (times do not depend on the values: no refill between reps)
            torch.cuda.synchronize()
            row("gae-inplace, product kernel", *timed(in_place, args.reps), tot * BYTES["gae-inplace"])
            gae(product, T, n, r0, d, None, None, adv, None)
            torch.cuda.synchronize()
            row("lean, product kernel", *timed(lambda: gae(product, T, n, r0, d, None, None, adv, None), args.reps), tot * BYTES["lean"])
            for key, lib in variants.items():
                gae(lib, T, n, r0, d, v0, vlast, adv, ret)
                torch.cuda.synchronize()
                row(f"gae V = 4, U = {key[0]} {HINT[key[1]]}", *timed(lambda: gae(lib, T, n, r0, d, v0, vlast, adv, ret), args.reps),
                    tot * BYTES["gae"])
            for key, lib in variants.items():
                gae(lib, T, n, r0, d, None, None, adv, None)
                torch.cuda.synchronize()
                row(f"lean V = 4, U = {key[0]} {HINT[key[1]]}", *timed(lambda: gae(lib, T, n, r0, d, None, None, adv, None), args.reps),
                    tot * BYTES["lean"])
            for key, lib in variants.items():
                r_ip.copy_(r0); v_ip.copy_(v0)
                gae(lib, T, n, r_ip, d, v_ip, vlast, r_ip, v_ip)
                torch.cuda.synchronize()
                row(f"gae-inplace V = 4, U = {key[0]} {HINT[key[1]]}", *timed(lambda: gae(lib, T, n, r_ip, d, v_ip, vlast, r_ip, v_ip), args.reps),
                    tot * BYTES["gae-inplace"])
            # V = 1 at the same shape: an advantage array one element off its 16-byte boundary is all it takes
            adv1 = torch.empty(T * n + 1, device="cuda")[1:].view(T, n)
            for key, lib in variants.items():
                gae(lib, T, n, r0, d, v0, vlast, adv1, ret)
                torch.cuda.synchronize()
                row(f"gae V = 1, U = {key[0]} {HINT[key[1]]}", *timed(lambda: gae(lib, T, n, r0, d, v0, vlast, adv1, ret), args.reps),
                    tot * BYTES["gae"])
            for key, lib in variants.items():
                gae(lib, T, n, r0, d, None, None, adv1, None)
                torch.cuda.synchronize()
                row(f"lean V = 1, U = {key[0]} {HINT[key[1]]}", *timed(lambda: gae(lib, T, n, r0, d, None, None, adv1, None), args.reps),
                    tot * BYTES["lean"])
            del adv1
        del r0, v0, d, adv, ret, adv_ref, ret_ref, r_ip, v_ip
        torch.cuda.empty_cache()
    # where V = 1 (four times the threads) overtakes V = 4: gae at T = 256 over lane counts, the non-temporal candidates (built without a threshold)
    T = 256
    lines.append(f"V = 4 against V = 1 over lane counts, gae, T = {T}, non-temporal candidates (us, median of {args.reps})")
    print(lines[-1], flush=True)
    for p in range(args.passes):
        for lg in (10, 12, 14, 16, 17, 18, 20):
            n = 1 << lg
            r0, v0, ret = (torch.randn((T, n), device="cuda") for _ in range(3))
            vlast = torch.randn((n,), device="cuda")
            d = (torch.rand((T, n), device="cuda") < 0.02).to(torch.uint8)
            adv = torch.empty((T, n), device="cuda")
            adv1 = torch.empty(T * n + 1, device="cuda")[1:].view(T, n)
            cells = []
            for u in (2, 4, 8):
                lib = variants[(u, 3)]
                for a in (adv, adv1):
                    gae(lib, T, n, r0, d, v0, vlast, a, ret)
                    torch.cuda.synchronize()
                    cells.append(timed(lambda: gae(lib, T, n, r0, d, v0, vlast, a, ret), args.reps)[0])
            line = (f"  pass {p + 1} lanes 2^{lg:2d}:  " + "   ".join(f"U = {u}: V4 {cells[2 * k]:8.1f}  V1 {cells[2 * k + 1]:8.1f}" for k, u in enumerate((2, 4, 8))))
            print(line, flush=True)
            lines.append(line)
            del r0, v0, ret, vlast, d, adv, adv1
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
