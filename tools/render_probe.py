"""Times gymnet_vecenv_render_device (gym.net_amd/csrc/render.hip) with HIP events against a hipMemsetAsync of the same bytes in the
same process: the frames' bytes written are the cost floor of the render.

    python tools/render_probe.py [--reps 20] [--out profiles/render_probe.txt]

Cases: GRAY8 40x20 (the Images runner's crop (200, 150, 200, 150)) at 2^20 lanes, GRAY8 84x84 of the full canvas at 2^16 lanes,
RGB8 600x400 at 1 and 64 lanes.  Per case: us per call (median of --reps timed windows of one call each), written GB/s, the fraction
of 8 TB/s, and the memset's time for the same bytes.  Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
CASES = [("gray8 40x20 crop", "gray", 1 << 20, (200, 150, 200, 150), (40, 20)),
         ("gray8 84x84 full", "gray", 1 << 16, (0, 0, 600, 400), (84, 84)),
         ("rgb8 600x400", "rgb", 1, (0, 0, 600, 400), (600, 400)),
         ("rgb8 600x400", "rgb", 64, (0, 0, 600, 400), (600, 400))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if pkg.device_count() < 1:
        raise SystemExit("render_probe: no GPU")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    stream = torch.cuda.Stream()              # the handle, the memset and the events share this stream (not the null stream: a
    torch.cuda.set_stream(stream)             # handle given stream 0 would create a stream of its own)
    rng = np.random.default_rng(0)
    lines, rows = [], []

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return float(np.median(ts))

    for name, fmt, n, crop, size in CASES:
        frame = size[0] * size[1] * (3 if fmt == "rgb" else 1)
        nbytes = n * frame
        out = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        with pkg.VectorEnv("CartPole-v1", n, seed=1, stream=stream.cuda_stream) as env:
            env.Reset()
            s = np.stack([rng.uniform(-2.4, 2.4, n), np.zeros(n), rng.uniform(-0.21, 0.21, n), np.zeros(n)]).astype(np.float32)
            env.SetState(s)
            us = timed(lambda: env.RenderDevice(out, fmt, crop=crop, size=size))
        ms = timed(lambda: hip.hipMemsetAsync(C.c_void_p(out.data_ptr()), 0, nbytes, C.c_void_p(stream.cuda_stream)))
        row = {"case": name, "lanes": n, "bytes": nbytes, "render_us": round(us, 2), "render_GBps": round(nbytes / us * 1e-3, 1),
               "render_frac_8TBps": round(nbytes / (us * 1e-6) / PEAK, 4), "memset_us": round(ms, 2),
               "memset_GBps": round(nbytes / ms * 1e-3, 1), "render_over_memset": round(us / ms, 2)}
        rows.append(row)
        lines.append(f"{name:18s} lanes {n:8d}  {nbytes / 1e6:9.2f} MB  render {us:10.2f} us  {row['render_GBps']:8.1f} GB/s "
                     f"({100 * row['render_frac_8TBps']:5.1f} % of 8 TB/s)  memset {ms:9.2f} us  render/memset {row['render_over_memset']:.2f}x")
        del out
    text = "\n".join(lines) + "\n" + json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, "cases": rows}) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
