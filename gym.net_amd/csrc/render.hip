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
#include "cartpole_raster.hpp"

namespace gymnet {

namespace {

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
    const int64_t frame_px = (int64_t)a.out_w * a.out_h;
    const int64_t frame_bytes = frame_px * C;
    for (int64_t w = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); w < a.total_waves; w += nwaves) {
        const int64_t k = w / a.waves_per_frame;                        // frame (wave-uniform)
        const int64_t slice = w - k * a.waves_per_frame;
        const Geo g = lane_geometry(static_cast<const R *>(a.obs), a.obs_stride, a.first_lane + k);
        const int64_t p0 = slice * kPixPerWave + (int64_t)lid * kPixPerThread;
        if (p0 >= frame_px) continue;
        uint8_t *frame = a.out + k * a.lane_stride;
        int i = (int)(p0 / a.out_w), j = (int)(p0 - (int64_t)i * a.out_w);
        PixelBytes<C> px;
#pragma unroll 1
        for (int q = 0; q < kPixPerThread; ++q) {
            int nw, np;
            shade(g, a.x0, a.sxq, a.y0, a.syq, i, j, nw, np);
            px.push(nw, np);
            if (++j == a.out_w) { j = 0; ++i; }
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

}  // namespace

int64_t render_waves_per_frame(int32_t out_w, int32_t out_h) { return ((int64_t)out_w * out_h + kPixPerWave - 1) / kPixPerWave; }

hipError_t launch_render(bool f64, int channels, const RenderArgs &a, hipStream_t st) {
    return f64 ? launch_render_typed<double>(channels, a, st) : launch_render_typed<float>(channels, a, st);
}

}  // namespace gymnet
