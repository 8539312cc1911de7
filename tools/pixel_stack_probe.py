"""Times gymnet_vecenv_pixel_stack_push_device (gym.net_amd/csrc/pixel_stack.hip) with HIP events in one process, beside what it fuses:
RenderDevice GRAY8 of the same frames (the newest frames alone) and a device-to-device copy that moves as many bytes as the push (it reads
depth - 1 slots and writes depth slots per lane; the copy reads and writes half of that each).

    python tools/pixel_stack_probe.py [--reps 10] [--max-gb 64] [--out profiles/pixel_stack_probe.txt]

Cases: 2^16 and 2^20 lanes x depth 2 and 4 x GRAY8 / BINARY8 / BINARY_F32 x the Images runner's shape (crop (200, 150, 200, 150) ->
40 x 20) and an 84 x 84 frame of the full canvas.  A case whose stack plus copy buffer exceeds --max-gb of device memory is listed as
not measured.  Per case: us per call (median of --reps windows of one call each) and push / render.  Needs a GPU; no fallback."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("runner 40x20", (200, 150, 200, 150), (40, 20)), ("full 84x84", (0, 0, 600, 400), (84, 84))]
FORMATS = [("gray8", 1), ("binary8", 1), ("binary_f32", 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max-gb", type=float, default=64.0)
    ap.add_argument("--lanes", default="16,20", help="log2 lane counts")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if pkg.device_count() < 1:
        raise SystemExit("pixel_stack_probe: no GPU")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.Stream()              # the handle, the copy and the events share this stream
    torch.cuda.set_stream(stream)
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

    for lg in (int(v) for v in args.lanes.split(",")):
        n = 1 << lg
        with pkg.VectorEnv("CartPole-v1", n, seed=1, auto_reset=True, stream=stream.cuda_stream) as env:
            env.Reset()
            s = np.stack([rng.uniform(-2.4, 2.4, n), np.zeros(n), rng.uniform(-0.21, 0.21, n), np.zeros(n)]).astype(np.float32)
            env.SetState(s)
            no_done = torch.zeros(n, dtype=torch.uint8, device="cuda")
            for shape, crop, size in SHAPES:
                frame_px = size[0] * size[1]
                for depth in (2, 4):
                    for fmt, elem in FORMATS:
                        frame = frame_px * elem
                        moved = (2 * depth - 1) * frame * n                  # bytes the push reads + writes
                        copy = moved // 2
                        need = depth * frame * n + copy
                        row = {"lanes": n, "shape": shape, "depth": depth, "format": fmt, "push_bytes": moved}
                        if need > args.max_gb * 1e9:
                            row["not_measured"] = f"needs {need / 1e9:.1f} GB of device memory (> {args.max_gb} GB)"
                            rows.append(row)
                            lines.append(f"2^{lg} {shape:13s} depth {depth} {fmt:10s}  not measured: {row['not_measured']}")
                            continue
                        st = env.PixelStack(depth=depth, size=size, crop=crop, format=fmt)
                        scratch = torch.empty(copy, dtype=torch.uint8, device="cuda")
                        push_us = timed(lambda: st.Push(no_done))
                        base = st.Tensor.data_ptr()
                        render_us = timed(lambda: env.RenderDevice(base, "gray", crop=crop, size=size,
                                                                   lane_stride=depth * frame))
                        copy_us = timed(lambda: hip.hipMemcpyAsync(C.c_void_p(scratch.data_ptr()), C.c_void_p(base), copy, 3,
                                                                    C.c_void_p(stream.cuda_stream)))
                        st.Close()
                        del st, scratch
                        torch.cuda.synchronize()
                        torch.cuda.empty_cache()
                        row.update({"push_us": round(push_us, 2), "render_gray8_us": round(render_us, 2), "copy_us": round(copy_us, 2),
                                    "push_over_render": round(push_us / render_us, 3), "push_GBps": round(moved / push_us * 1e-3, 1),
                                    "copy_GBps": round(2 * copy / copy_us * 1e-3, 1)})
                        rows.append(row)
                        lines.append(f"2^{lg} {shape:13s} depth {depth} {fmt:10s}  push {push_us:10.2f} us  render {render_us:10.2f} us  "
                                     f"push/render {row['push_over_render']:5.3f}  copy of the same bytes {copy_us:10.2f} us  "
                                     f"({moved / 1e9:7.3f} GB moved)")
                        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n" + json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, "cases": rows}) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
