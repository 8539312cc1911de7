// pixel_stack.hip — episode-aware stacks of processed CartPole frames, kept on the device per lane (the Images runner's 2-deep frame
// queue, ReplayMemory.cs:38-54, and its input transform, ImageDataBuilder.cs:10-18).  The contract is gymnet_vecenv_pixel_stack_config /
// _push_device / _reset_device in include/gymnet_amd.h; tests/_pixel_stack_model.py restates it in NumPy.  Written for gfx950 (wave64);
// compiled with -ffp-contract=off.
//
// Layout of the work is render.hip's: one wave covers 1024 consecutive pixels of ONE lane's frame (16 per thread), the lane geometry is
// computed once per wave, and a thread shades its 16 pixels with the same shade() render_kernel uses.  A thread owns its 16 pixel
// positions in EVERY slot of the lane's stack: it first issues the loads of the older slots it moves (they are in flight while it
// shades), then stores slot s from the old slot s + 1 and the new frame into the newest slot.  Shifting in place is race-free because
// no other thread reads or writes those positions of any slot.  A restarting lane (wave-uniform) loads nothing and stores the new frame
// into every slot; reset_device is the same kernel with the shift switched off and the lanes outside the mask left alone.
// Stores are dwordx4 when the slot start is 16-byte aligned (a BINARY_F32 thread writes 64 bytes per slot), bytes (dwords for
// BINARY_F32) at a frame's tail or in a slot that is not aligned.
//
// The host side follows the kernel: gymnet_vecenv_pixel_stack_* and the handle's PixelStack attachment.
#include "cartpole_raster.hpp"
#include "handle.hpp"

namespace gymnet {

namespace {

// Lane k's stack at base + k * lane_stride, slot s at + s * frame_bytes, every slot one frame of geo.out_h x geo.out_w pixels drawn as
// render_kernel draws it (format GYMNET_STACK_*: GRAY8, BINARY8 or BINARY_F32).
struct StackArgs {
    const void *obs; int64_t obs_stride;      // the CURRENT observation buffer [4][obs_stride], float or double
    uint8_t *base; int64_t lane_stride, frame_bytes;
    // shift = 1 (push): slots 0..depth-2 take the old slots 1..depth-1 and the newest takes the frame, except in lanes with
    // restart[k] != 0 (no array: none), which take the frame in every slot.  shift = 0 (reset): lanes with restart[k] != 0 (no array:
    // every lane) take the frame in every slot, the others are not touched.
    const uint8_t *restart;
    int32_t depth, shift;
    int64_t total_waves;                      // num_envs * geo.waves_per_frame
    FrameGeom geo;
};

__device__ __forceinline__ bool at16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// 16 pixels of E bytes in stream order: 4 * E dwords
template <int E>
__device__ __forceinline__ void append(uint32_t (&w)[4 * E], uint32_t v) {
    if constexpr (E == 1) {
        w[0] = __builtin_amdgcn_alignbyte(w[1], w[0], 1);
        w[1] = __builtin_amdgcn_alignbyte(w[2], w[1], 1);
        w[2] = __builtin_amdgcn_alignbyte(w[3], w[2], 1);
        w[3] = __builtin_amdgcn_alignbyte(v, w[3], 1);
    } else {
#pragma unroll
        for (int k = 0; k < 15; ++k) w[k] = w[k + 1];
        w[15] = v;
    }
}

// A thread's 16 E bytes of one slot at slot + b0.  vec: the slot start is 16-byte aligned and all 16 E bytes lie inside the frame;
// otherwise only the first m bytes are touched (E = 4: slots are 4-byte aligned and m a multiple of 4, so dwords).
template <int E>
__device__ __forceinline__ void load_px(const uint8_t *slot, int64_t b0, int m, bool vec, uint32_t (&w)[4 * E]) {
    if (vec) {
        const uint4 *src = reinterpret_cast<const uint4 *>(slot + b0);
#pragma unroll
        for (int v = 0; v < E; ++v) {
            const uint4 q = src[v];
            w[4 * v] = q.x; w[4 * v + 1] = q.y; w[4 * v + 2] = q.z; w[4 * v + 3] = q.w;
        }
    } else if constexpr (E == 4) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(slot + b0);
#pragma unroll
        for (int v = 0; v < 16; ++v) w[v] = 4 * v < m ? src[v] : 0u;
    } else {
        w[0] = w[1] = w[2] = w[3] = 0u;
#pragma unroll
        for (int v = 0; v < 16; ++v)
            if (v < m) w[v >> 2] |= (uint32_t)slot[b0 + v] << (8 * (v & 3));
    }
}

template <int E>
__device__ __forceinline__ void store_px(uint8_t *slot, int64_t b0, int m, bool vec, const uint32_t (&w)[4 * E]) {
    if (vec) {
        uint4 *dst = reinterpret_cast<uint4 *>(slot + b0);
#pragma unroll
        for (int v = 0; v < E; ++v) dst[v] = make_uint4(w[4 * v], w[4 * v + 1], w[4 * v + 2], w[4 * v + 3]);
    } else if constexpr (E == 4) {
        uint32_t *dst = reinterpret_cast<uint32_t *>(slot + b0);
#pragma unroll
        for (int v = 0; v < 16; ++v)
            if (4 * v < m) dst[v] = w[v];
    } else {
#pragma unroll
        for (int v = 0; v < 16; ++v)
            if (v < m) slot[b0 + v] = (uint8_t)(w[v >> 2] >> (8 * (v & 3)));
    }
}

template <class R, int FMT>
__global__ __launch_bounds__(256) void pixel_stack_kernel(StackArgs a) {
    constexpr int E = FMT == GYMNET_STACK_BINARY_F32 ? 4 : 1;      // bytes per pixel
    constexpr int kAhead = 3;                   // older slots whose loads are issued before the shading (12 / 48 VGPRs); deeper stacks
                                                // move the rest one slot at a time after it
    const int lid = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int64_t frame_px = (int64_t)a.geo.out_w * a.geo.out_h;
    for (int64_t w = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); w < a.total_waves; w += nwaves) {
        const int64_t k = w / a.geo.waves_per_frame;                        // lane (wave-uniform)
        const int64_t slice = w - k * a.geo.waves_per_frame;
        // push: a lane restarts where restart[k] != 0 (none without the array); reset: the masked lanes (all without a mask) restart
        // and the others are left alone
        const int flag = a.restart ? __builtin_amdgcn_readfirstlane((int)a.restart[k]) : (a.shift ? 0 : 1);
        if (!a.shift && !flag) continue;
        const bool restart = flag != 0;
        const int64_t p0 = slice * kPixPerWave + (int64_t)lid * kPixPerThread;
        if (p0 >= frame_px) continue;
        uint8_t *stack = a.base + k * a.lane_stride;
        const int64_t b0 = p0 * E;
        const int64_t nb = a.frame_bytes - b0;                         // bytes of the frame from b0 on (> 0)
        const int m = nb < 16 * E ? (int)nb : 16 * E;
        const bool whole = nb >= 16 * E;
        const int nold = restart ? 0 : a.depth - 1;                    // older slots that move down one
        uint32_t old[kAhead][4 * E];
#pragma unroll
        for (int s = 0; s < kAhead; ++s)
            if (s < nold) {
                const uint8_t *src = stack + (int64_t)(s + 1) * a.frame_bytes;
                load_px<E>(src, b0, m, whole && at16(src), old[s]);
            }
        const Geo g = lane_geometry(static_cast<const R *>(a.obs), a.obs_stride, k);
        int i = (int)(p0 / a.geo.out_w), j = (int)(p0 - (int64_t)i * a.geo.out_w);
        uint32_t px[4 * E];
#pragma unroll
        for (int v = 0; v < 4 * E; ++v) px[v] = 0u;
#pragma unroll 1
        for (int q = 0; q < kPixPerThread; ++q) {
            int nw, np;
            shade(g, a.geo.x0, a.geo.sxq, a.geo.y0, a.geo.syq, i, j, nw, np);
            append<E>(px, stack_value<FMT>(nw, np));
            if (++j == a.geo.out_w) { j = 0; ++i; }
        }
#pragma unroll
        for (int s = 0; s < kAhead; ++s)
            if (s < nold) {
                uint8_t *dst = stack + (int64_t)s * a.frame_bytes;
                store_px<E>(dst, b0, m, whole && at16(dst), old[s]);
            }
#pragma unroll 1
        for (int s = kAhead; s < nold; ++s) {
            uint32_t t[4 * E];
            const uint8_t *src = stack + (int64_t)(s + 1) * a.frame_bytes;
            uint8_t *dst = stack + (int64_t)s * a.frame_bytes;
            load_px<E>(src, b0, m, whole && at16(src), t);
            store_px<E>(dst, b0, m, whole && at16(dst), t);
        }
#pragma unroll 1
        for (int s = restart ? 0 : a.depth - 1; s < a.depth; ++s) {
            uint8_t *dst = stack + (int64_t)s * a.frame_bytes;
            store_px<E>(dst, b0, m, whole && at16(dst), px);
        }
    }
}

template <class R>
hipError_t launch_pixel_stack_typed(int32_t format, const StackArgs &a, hipStream_t st) {
    // a grid-stride loop over the (lane, slice) waves: at most 2^20 workgroups of 4 waves in flight per launch
    const int64_t blocks = (a.total_waves + 3) / 4;
    const unsigned grid = (unsigned)(blocks < (int64_t)1 << 20 ? blocks : (int64_t)1 << 20);
    if (format == GYMNET_STACK_GRAY8) hipLaunchKernelGGL((pixel_stack_kernel<R, GYMNET_STACK_GRAY8>), dim3(grid), dim3(256), 0, st, a);
    else if (format == GYMNET_STACK_BINARY8) hipLaunchKernelGGL((pixel_stack_kernel<R, GYMNET_STACK_BINARY8>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((pixel_stack_kernel<R, GYMNET_STACK_BINARY_F32>), dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

constexpr int32_t kStackMaxDepth = 64;

}  // namespace

// the configured stack: args.obs / restart / shift are filled in per launch; mem holds the stack when the handle allocated it (empty: adopted)
struct PixelStack { DeviceAllocs mem; StackArgs args{}; int32_t format = 0; };

int release_stack(gymnet_vecenv *h) { return release_attachment(h, h->stack); }

namespace {

int need_stack(gymnet_vecenv *h) {
    return h->stack ? GYMNET_OK : fail(h, GYMNET_ERR_INVALID_ARG, "no pixel stack configured (gymnet_vecenv_pixel_stack_config)");
}

// one launch over every lane of the configured stack, from the CURRENT observation buffer: shift = 1 push, 0 reset (StackArgs)
int launch_stack(gymnet_vecenv *h, const uint8_t *restart, int32_t shift) {
    StackArgs a = h->stack->args;
    a.obs = h->d_obs; a.obs_stride = h->ostride;
    a.restart = restart; a.shift = shift;
    HIP_TRY(h, h->f64 ? launch_pixel_stack_typed<double>(h->stack->format, a, h->stream) : launch_pixel_stack_typed<float>(h->stack->format, a, h->stream));
    return GYMNET_OK;
}

}  // namespace

}  // namespace gymnet

using namespace gymnet;

extern "C" {

int gymnet_vecenv_pixel_stack_config(gymnet_vecenv *h, int32_t format, int32_t depth, int32_t crop_x, int32_t crop_y, int32_t crop_w,
                                     int32_t crop_h, int32_t out_w, int32_t out_h, void *d_ext, int64_t lane_stride) {
    return guarded([&]() -> int {
    ENTER(h);
    if (h->cfg.env_id != GYMNET_ENV_CARTPOLE) return fail(h, GYMNET_ERR_UNSUPPORTED, "pixel stacks exist for CartPole only (CartPoleEnv.cs:69-135)");
    if (depth == 0) return release_stack(h);
    if (format != GYMNET_STACK_GRAY8 && format != GYMNET_STACK_BINARY8 && format != GYMNET_STACK_BINARY_F32)
        return fail(h, GYMNET_ERR_INVALID_ARG, "unknown pixel stack format %d", format);
    if (depth < 0 || depth > kStackMaxDepth) return fail(h, GYMNET_ERR_INVALID_ARG, "depth %d not in [0, %d]", depth, kStackMaxDepth);
    ST_TRY(check_crop_and_size(h, crop_x, crop_y, crop_w, crop_h, out_w, out_h));
    const int64_t elem = format == GYMNET_STACK_BINARY_F32 ? 4 : 1;
    const int64_t frame = (int64_t)out_w * out_h * elem, span = (int64_t)depth * frame;
    if (lane_stride == 0) lane_stride = span;
    if (lane_stride < span)
        return fail(h, GYMNET_ERR_INVALID_ARG, "lane_stride %lld < %lld bytes of one stack", (long long)lane_stride, (long long)span);
    if (h->n > 1 && lane_stride > (INT64_MAX - span) / (h->n - 1)) return fail(h, GYMNET_ERR_INVALID_ARG, "num_envs x lane_stride overflows");
    if (elem == 4 && ((reinterpret_cast<uintptr_t>(d_ext) & 3u) != 0 || lane_stride % 4 != 0))
        return fail(h, GYMNET_ERR_INVALID_ARG, "BINARY_F32 stacks need a 4-byte aligned d_ext and lane_stride");
    const int64_t bytes = (h->n - 1) * lane_stride + span;
    std::unique_ptr<PixelStack> fresh(new PixelStack);
    if (!d_ext && !(d_ext = fresh->mem.take((size_t)bytes)))
        return fail(h, GYMNET_ERR_OOM, "hipMalloc(%lld bytes) for the pixel stack failed", (long long)bytes);
    StackArgs &a = fresh->args;
    a.base = static_cast<uint8_t *>(d_ext);
    a.lane_stride = lane_stride; a.frame_bytes = frame;
    a.depth = depth;
    a.geo = frame_geom(crop_x, crop_y, crop_w, crop_h, out_w, out_h);
    a.total_waves = h->n * a.geo.waves_per_frame;
    fresh->format = format;
    ST_TRY(release_stack(h));
    h->stack = fresh.release();
    return launch_stack(h, nullptr, 0);
    });
}

int gymnet_vecenv_pixel_stack_reset_device(gymnet_vecenv *h, const uint8_t *d_mask) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_stack(h));
    return launch_stack(h, d_mask, 0);
    });
}

int gymnet_vecenv_pixel_stack_push_device(gymnet_vecenv *h, const uint8_t *d_done) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_stack(h));
    // without a done array an auto-reset handle restarts the lanes its most recent step finished (and already re-drew)
    return launch_stack(h, d_done ? d_done : (h->autoreset ? h->d_done : nullptr), 1);
    });
}

int gymnet_vecenv_pixel_stack_view(gymnet_vecenv *h, void **d_stack, int64_t *lane_stride, int64_t *frame_bytes) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_stack(h));
    if (d_stack) *d_stack = h->stack->args.base;
    if (lane_stride) *lane_stride = h->stack->args.lane_stride;
    if (frame_bytes) *frame_bytes = h->stack->args.frame_bytes;
    return GYMNET_OK;
    });
}

int gymnet_vecenv_pixel_stack_read(gymnet_vecenv *h, void *out, int64_t first_lane, int64_t count) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_stack(h));
    if (!out) return fail(h, GYMNET_ERR_INVALID_ARG, "out is null");
    if (first_lane < 0 || count < 1 || first_lane > h->n - count)
        return fail(h, GYMNET_ERR_INVALID_ARG, "lanes [%lld, %lld + %lld) not inside [0, %lld)", (long long)first_lane, (long long)first_lane,
                    (long long)count, (long long)h->n);
    const StackArgs &a = h->stack->args;
    const int64_t span = (int64_t)a.depth * a.frame_bytes;
    const uint8_t *src = a.base + first_lane * a.lane_stride;
    if (a.lane_stride == span) HIP_TRY(h, hipMemcpyAsync(out, src, (size_t)(count * span), hipMemcpyDeviceToHost, h->stream));
    else HIP_TRY(h, hipMemcpy2DAsync(out, (size_t)span, src, (size_t)a.lane_stride, (size_t)span, (size_t)count, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GYMNET_OK;
    });
}

}  // extern "C"
