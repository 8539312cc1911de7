// render.hip — CartPole frames rasterised straight from the handle's current observation buffer (CartPoleEnv.Render,
// CartPoleEnv.cs:69-135): the reference's 600x400 canvas, its shapes and colours, 4x4-supersampled into RGB8 or GRAY8 frames of any
// crop and output size.  The contract (geometry, paint order, sample positions, rounding) is gymnet_vecenv_render_device in
// include/gymnet_amd.h; tests/_render_twin.py restates it in NumPy.  Written for gfx950 (wave64); compiled with -ffp-contract=off.
//
// Layout of the work: a frame is one flat byte run of out_w * out_h * C bytes (C = 3 or 1).  One wave covers 1024 consecutive pixels of
// ONE frame (16 per thread, so a thread's bytes are 16 (GRAY8) or 48 (RGB8) contiguous bytes: dwordx4 stores whenever the frame start is
// 16-byte aligned, byte stores only at a frame's tail).  Everything that depends on the lane alone — cart position, sin / cos of the pole
// angle, the shapes' bounding box — is computed once per wave from two wave-uniform loads.  Per pixel, a sample row that misses the
// bounding box costs two compares (it is background or track); only rows that cross the box test their four samples against the shapes.
//
// The host side follows the kernels: gymnet_vecenv_render / _render_device, the crop rules every frame request shares, and the device
// staging of the host-boundary call (the handle's RenderStaging attachment).
#include <cstring>

#include "cartpole_raster.hpp"
#include "handle.hpp"

namespace gymnet {

// gymnet_vecenv_render's device staging (allocated on first use, grown on demand)
struct RenderStaging { DeviceAllocs mem; size_t cap = 0; };

namespace {

// Frame k of lanes [first_lane, first_lane + count) is out + k * lane_stride; total_waves = count * geo.waves_per_frame.
struct RenderArgs {
    const void *obs; int64_t obs_stride;      // the CURRENT observation buffer [4][obs_stride], float or double
    int64_t first_lane;
    uint8_t *out; int64_t lane_stride;
    int64_t total_waves;
    FrameGeom geo;
};

template <int C> struct PixelBytes;                        // 16 pixels of C bytes each, as 4 * C dwords in stream order
template <> struct PixelBytes<1> {
    uint32_t w[4] = {0, 0, 0, 0};
    __device__ __forceinline__ void push(int nw, int np) {     // BT.709 luma, rounded: white 255, black 0, pole / axle 160
        const uint32_t y = (uint32_t)(nw * 255 + np * 160 + 8) >> 4;
        w[0] = __builtin_amdgcn_alignbyte(w[1], w[0], 1);
        w[1] = __builtin_amdgcn_alignbyte(w[2], w[1], 1);
        w[2] = __builtin_amdgcn_alignbyte(w[3], w[2], 1);
        w[3] = __builtin_amdgcn_alignbyte(y, w[3], 1);
    }
};
template <> struct PixelBytes<3> {
    uint32_t w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    __device__ __forceinline__ void push(int nw, int np) {     // white (255, 255, 255), black (0, 0, 0), pole / axle (204, 153, 102)
        const uint32_t r = (uint32_t)(nw * 255 + np * 204 + 8) >> 4;
        const uint32_t gg = (uint32_t)(nw * 255 + np * 153 + 8) >> 4;
        const uint32_t b = (uint32_t)(nw * 255 + np * 102 + 8) >> 4;
        const uint32_t rgb = r | (gg << 8) | (b << 16);
#pragma unroll
        for (int k = 0; k < 11; ++k) w[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], 3);
        w[11] = __builtin_amdgcn_alignbyte(rgb, w[11], 3);
    }
};

template <class R, int C>
__global__ __launch_bounds__(256) void render_kernel(RenderArgs a) {
    const int lid = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int64_t frame_px = (int64_t)a.geo.out_w * a.geo.out_h;
    const int64_t frame_bytes = frame_px * C;
    for (int64_t w = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); w < a.total_waves; w += nwaves) {
        const int64_t k = w / a.geo.waves_per_frame;                        // frame (wave-uniform)
        const int64_t slice = w - k * a.geo.waves_per_frame;
        const Geo g = lane_geometry(static_cast<const R *>(a.obs), a.obs_stride, a.first_lane + k);
        const int64_t p0 = slice * kPixPerWave + (int64_t)lid * kPixPerThread;
        if (p0 >= frame_px) continue;
        uint8_t *frame = a.out + k * a.lane_stride;
        int i = (int)(p0 / a.geo.out_w), j = (int)(p0 - (int64_t)i * a.geo.out_w);
        PixelBytes<C> px;
#pragma unroll 1
        for (int q = 0; q < kPixPerThread; ++q) {
            int nw, np;
            shade(g, a.geo.x0, a.geo.sxq, a.geo.y0, a.geo.syq, i, j, nw, np);
            px.push(nw, np);
            if (++j == a.geo.out_w) { j = 0; ++i; }
        }
        const int64_t b0 = p0 * C;
        const int64_t nb = frame_bytes - b0;                           // bytes of this frame from b0 on (> 0)
        if (nb >= 16 * C && (reinterpret_cast<uintptr_t>(frame) & 15u) == 0) {
            uint4 *dst = reinterpret_cast<uint4 *>(frame + b0);
#pragma unroll
            for (int v = 0; v < C; ++v) dst[v] = make_uint4(px.w[4 * v], px.w[4 * v + 1], px.w[4 * v + 2], px.w[4 * v + 3]);
        } else {
            const int m = nb < 16 * C ? (int)nb : 16 * C;
#pragma unroll
            for (int v = 0; v < 16 * C; ++v)
                if (v < m) frame[b0 + v] = (uint8_t)(px.w[v >> 2] >> (8 * (v & 3)));
        }
    }
}

template <class R>
hipError_t launch_render_typed(int channels, const RenderArgs &a, hipStream_t st) {
    // a grid-stride loop over the (frame, slice) waves: at most 2^20 workgroups of 4 waves in flight per launch
    const int64_t blocks = (a.total_waves + 3) / 4;
    const unsigned grid = (unsigned)(blocks < (int64_t)1 << 20 ? blocks : (int64_t)1 << 20);
    if (channels == 3) hipLaunchKernelGGL((render_kernel<R, 3>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((render_kernel<R, 1>), dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_render(gymnet_vecenv *h, int32_t format, const RenderArgs &a) {
    const int channels = format == GYMNET_PIXELS_RGB8 ? 3 : 1;
    return h->f64 ? launch_render_typed<double>(channels, a, h->stream) : launch_render_typed<float>(channels, a, h->stream);
}

// Checks a render request (nothing is written on failure) and fills the kernel arguments; *bytes = the span the frames cover.
int render_args(gymnet_vecenv *h, void *out, int32_t format, int64_t first_lane, int64_t count, int32_t crop_x, int32_t crop_y,
                int32_t crop_w, int32_t crop_h, int32_t out_w, int32_t out_h, int64_t lane_stride, RenderArgs *a, int64_t *bytes) {
    if (h->cfg.env_id != GYMNET_ENV_CARTPOLE) return fail(h, GYMNET_ERR_UNSUPPORTED, "rendering exists for CartPole only (CartPoleEnv.cs:69-135)");
    if (!out) return fail(h, GYMNET_ERR_INVALID_ARG, "out is null");
    if (format != GYMNET_PIXELS_RGB8 && format != GYMNET_PIXELS_GRAY8) return fail(h, GYMNET_ERR_INVALID_ARG, "unknown pixel format %d", format);
    if (first_lane < 0 || count < 1 || first_lane > h->n - count)
        return fail(h, GYMNET_ERR_INVALID_ARG, "lanes [%lld, %lld + %lld) not inside [0, %lld)", (long long)first_lane, (long long)first_lane,
                    (long long)count, (long long)h->n);
    ST_TRY(check_crop_and_size(h, crop_x, crop_y, crop_w, crop_h, out_w, out_h));
    const int64_t frame = (int64_t)out_w * out_h * (format == GYMNET_PIXELS_RGB8 ? 3 : 1);
    if (lane_stride < frame) return fail(h, GYMNET_ERR_INVALID_ARG, "lane_stride %lld < %lld bytes of one frame", (long long)lane_stride, (long long)frame);
    if (lane_stride > (INT64_MAX - frame) / count) return fail(h, GYMNET_ERR_INVALID_ARG, "count x lane_stride overflows");
    a->obs = h->d_obs; a->obs_stride = h->ostride;
    a->first_lane = first_lane;
    a->out = static_cast<uint8_t *>(out); a->lane_stride = lane_stride;
    a->geo = frame_geom(crop_x, crop_y, crop_w, crop_h, out_w, out_h);
    a->total_waves = count * a->geo.waves_per_frame;
    *bytes = (count - 1) * lane_stride + frame;
    return GYMNET_OK;
}

}  // namespace

int check_crop_and_size(gymnet_vecenv *h, int32_t crop_x, int32_t crop_y, int32_t crop_w, int32_t crop_h, int32_t out_w, int32_t out_h) {
    if (crop_w < 1 || crop_h < 1 || crop_x < 0 || crop_y < 0 || crop_x > kRenderWidth - crop_w || crop_y > kRenderHeight - crop_h)
        return fail(h, GYMNET_ERR_INVALID_ARG, "crop (%d, %d, %d, %d) not inside the %dx%d canvas", crop_x, crop_y, crop_w, crop_h, kRenderWidth, kRenderHeight);
    if (out_w < 1 || out_h < 1 || out_w > kRenderMaxSide || out_h > kRenderMaxSide)
        return fail(h, GYMNET_ERR_INVALID_ARG, "output size %dx%d not in [1, %d]", out_w, out_h, kRenderMaxSide);
    return GYMNET_OK;
}

int release_render(gymnet_vecenv *h) { return release_attachment(h, h->render); }

}  // namespace gymnet

using namespace gymnet;

extern "C" {

int gymnet_vecenv_render_device(gymnet_vecenv *h, void *d_out, int32_t format, int64_t first_lane, int64_t count, int32_t crop_x,
                                int32_t crop_y, int32_t crop_w, int32_t crop_h, int32_t out_w, int32_t out_h, int64_t lane_stride) {
    return guarded([&]() -> int {
    ENTER(h);
    RenderArgs a{};
    int64_t bytes = 0;
    ST_TRY(render_args(h, d_out, format, first_lane, count, crop_x, crop_y, crop_w, crop_h, out_w, out_h, lane_stride, &a, &bytes));
    HIP_TRY(h, launch_render(h, format, a));
    return GYMNET_OK;
    });
}

int gymnet_vecenv_render(gymnet_vecenv *h, void *out, int32_t format, int64_t first_lane, int64_t count, int32_t crop_x, int32_t crop_y,
                         int32_t crop_w, int32_t crop_h, int32_t out_w, int32_t out_h, int64_t lane_stride) {
    return guarded([&]() -> int {
    ENTER(h);
    RenderArgs a{};
    int64_t bytes = 0;
    ST_TRY(render_args(h, out, format, first_lane, count, crop_x, crop_y, crop_w, crop_h, out_w, out_h, lane_stride, &a, &bytes));
    if (!h->render || h->render->cap < (size_t)bytes) {
        std::unique_ptr<RenderStaging> fresh(new RenderStaging);
        if (!fresh->mem.take((size_t)bytes)) return fail(h, GYMNET_ERR_OOM, "hipMalloc(%lld bytes) for the render staging failed", (long long)bytes);
        fresh->cap = (size_t)bytes;
        ST_TRY(release_render(h));
        h->render = fresh.release();
    }
    uint8_t *staging = static_cast<uint8_t *>(h->render->mem.ptrs[0]);
    a.out = staging;
    HIP_TRY(h, launch_render(h, format, a));
    // only the frames' own bytes cross: the caller's gaps between them (lane_stride > one frame) stay as they were
    const int64_t frame = (int64_t)out_w * out_h * (format == GYMNET_PIXELS_RGB8 ? 3 : 1);
    if (lane_stride == frame) {
        HIP_TRY(h, hipMemcpyAsync(out, staging, (size_t)bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return GYMNET_OK;
    }
    std::vector<uint8_t> span((size_t)bytes);
    HIP_TRY(h, hipMemcpyAsync(span.data(), staging, (size_t)bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int64_t k = 0; k < count; ++k) std::memcpy(static_cast<uint8_t *>(out) + k * lane_stride, span.data() + k * lane_stride, (size_t)frame);
    return GYMNET_OK;
    });
}

}  // extern "C"
