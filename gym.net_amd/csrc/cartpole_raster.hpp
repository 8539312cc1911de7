// cartpole_raster.hpp — the CartPole canvas (CartPoleEnv.Render, CartPoleEnv.cs:69-135) as the frame kernels see it: the per-lane
// geometry a wave computes once (lane_geometry), the 16-sample coverage of one output pixel (shade) and a stack pixel's value
// (stack_value).  Shared by render.hip (frames), pixel_stack.hip (episode-aware frame stacks) and episode_memory.hip (dataset frames), so
// all of them draw the same pixels from the same arithmetic.  The contract is
// gymnet_vecenv_render_device in include/gymnet_amd.h; compiled with -ffp-contract=off like every unit.
//
// The work decomposition is shared too: one wave covers kPixPerWave consecutive pixels of ONE frame, kPixPerThread per thread.
#pragma once
#include "kernels.hpp"

#include "envs.hpp"
#include "../../include/gymnet_amd.h"

namespace gymnet {

constexpr int32_t kRenderWidth = 600, kRenderHeight = 400;   // the reference's canvas (CartPoleEnv.cs:71-72)
constexpr int32_t kRenderMaxSide = 16384;                    // output width / height limit (sample positions stay exact in float)

// What every frame kernel needs to know about its frames; embedded in each one's argument struct (render.hip, pixel_stack.hip,
// episode_memory.hip).  Sample (a, b) of pixel (i, j) is at x0 + (4 j + a + 0.5) * sxq, y0 + (4 i + b + 0.5) * syq.
struct FrameGeom { int64_t waves_per_frame; int32_t out_w, out_h; float x0, y0, sxq, syq; };
// the crop / output-size rules every frame request shares (gymnet_vecenv_render_device); render.hip
int check_crop_and_size(gymnet_vecenv *h, int32_t crop_x, int32_t crop_y, int32_t crop_w, int32_t crop_h, int32_t out_w, int32_t out_h);

namespace {

// CartPoleEnv.cs:69-135, the C# float constants: scale = screen_width / world_width, world_width = x_threshold * 2, polelen = scale * (2 * length)
constexpr float kScale = 600.0f / (2.4f * 2.0f);          // 124.99999237f
constexpr float kPoleLen = kScale * (2.0f * 0.5f);
constexpr float kPivotY = 295.0f;                         // the pole's pivot and the axle: 5 px above the track row (carty = 300)
constexpr float kVlo = 5.0f - kPoleLen;                   // pole rectangle in pole coordinates: u in [-5, 5], v in [5 - polelen, 5]
constexpr int kPixPerThread = 16;
constexpr int kPixPerWave = 64 * kPixPerThread;

inline int64_t render_waves_per_frame(int32_t out_w, int32_t out_h) { return ((int64_t)out_w * out_h + kPixPerWave - 1) / kPixPerWave; }
inline FrameGeom frame_geom(int32_t crop_x, int32_t crop_y, int32_t crop_w, int32_t crop_h, int32_t out_w, int32_t out_h) {
    return {render_waves_per_frame(out_w, out_h), out_w, out_h, (float)crop_x, (float)crop_y,
            (float)((double)crop_w / (4.0 * out_w)), (float)((double)crop_h / (4.0 * out_h))};
}

struct Geo {
    float cx, cl, cr;          // cart centre and its closed x-range [cx - 25, cx + 25]
    float c, s;                // cos / sin of the pole angle (0 when the angle is not finite)
    float vlo, vhi;            // the pole's v-range ([+inf, -inf]: no pole)
    float bx0, bx1, by0, by1;  // bounding box of cart + pole + axle, half a pixel of margin ([+inf, -inf]: nothing but track)
};

template <class R>
__device__ __forceinline__ Geo lane_geometry(const R *obs, int64_t ostride, int64_t lane) {
    Geo g;
    const R x = obs[lane], th = obs[2 * ostride + lane];
    g.cx = (float)((double)x * (double)kScale + 300.0);
    g.cl = g.cx - 25.0f;
    g.cr = g.cx + 25.0f;
    const float t = (float)th;
    g.c = 0.0f; g.s = 0.0f;
    g.vlo = INFINITY; g.vhi = -INFINITY;
    g.bx0 = INFINITY; g.bx1 = -INFINITY; g.by0 = INFINITY; g.by1 = -INFINITY;
    if (!isfinite(g.cx)) return g;                         // no cart, pole or axle: background and track only
    float dx0 = -25.0f, dx1 = 25.0f, dy0 = -10.0f, dy1 = 20.0f;     // the cart [285, 315] about the pivot row; contains the axle disc
    if (isfinite(t)) {
        sincos_f32(t, g.s, g.c);
        g.vlo = kVlo; g.vhi = 5.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {                      // pole corners: (dx, dy) = (u c - v s, u s + v c)
            const float u = (k & 1) ? 5.0f : -5.0f, v = (k & 2) ? 5.0f : kVlo;
            const float px = u * g.c - v * g.s, py = u * g.s + v * g.c;
            dx0 = fminf(dx0, px); dx1 = fmaxf(dx1, px); dy0 = fminf(dy0, py); dy1 = fmaxf(dy1, py);
        }
    }
    g.bx0 = g.cx + dx0 - 0.5f; g.bx1 = g.cx + dx1 + 0.5f;
    g.by0 = kPivotY + dy0 - 0.5f; g.by1 = kPivotY + dy1 + 0.5f;
    return g;
}

// One output pixel: how many of its 16 samples are white (background) and how many are pole colour (pole or axle); the rest are black
// (track or cart).  xs / ys of sample (a, b) = crop origin + (4 j + a + 0.5) * sxq, (4 i + b + 0.5) * syq with sxq = crop_w / (4 out_w).
__device__ __forceinline__ void shade(const Geo &g, float xs0, float sxq, float ys0, float syq, int i, int j, int &nw, int &np) {
    float xs[4], dx[4], dxc[4], dxs[4], dx2[4];
    bool cc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        xs[a] = xs0 + ((float)(4 * j + a) + 0.5f) * sxq;
        dx[a] = xs[a] - g.cx;
        dxc[a] = dx[a] * g.c; dxs[a] = dx[a] * g.s; dx2[a] = dx[a] * dx[a];
        cc[a] = (xs[a] >= g.cl) & (xs[a] <= g.cr);
    }
    const bool xin = (xs[3] >= g.bx0) & (xs[0] <= g.bx1);
    nw = 0; np = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const float ys = ys0 + ((float)(4 * i + b) + 0.5f) * syq;
        const bool track = (ys >= 300.0f) & (ys < 301.0f);
        if (xin & (ys >= g.by0) & (ys <= g.by1)) {
            const float dy = ys - kPivotY;
            const float dyc = dy * g.c, dys = dy * g.s, dy2 = dy * dy;
            const bool black_row = track | ((ys >= 285.0f) & (ys <= 315.0f));
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const float u = dxc[a] + dys, v = dyc - dxs[a];
                const bool pole = (fabsf(u) <= 5.0f) & (v >= g.vlo) & (v <= g.vhi);
                const bool axle = dx2[a] + dy2 <= 25.0f;
                const bool black = track | (black_row & cc[a]);
                np += (pole | axle) ? 1 : 0;
                nw += (pole | axle | black) ? 0 : 1;
            }
        } else {
            nw += track ? 0 : 4;
        }
    }
}

// what a pixel of the stack holds, from its shade() counts: the GRAY8 value of gymnet_vecenv_render_device, or 1 where that value is
// below 255 (a sample that is not background), as a byte or as 1.0f
template <int FMT>
__device__ __forceinline__ uint32_t stack_value(int nw, int np) {
    const uint32_t y = (uint32_t)(nw * 255 + np * 160 + 8) >> 4;
    if constexpr (FMT == GYMNET_STACK_GRAY8) return y;
    else if constexpr (FMT == GYMNET_STACK_BINARY8) return y < 255u ? 1u : 0u;
    else return y < 255u ? 0x3f800000u : 0u;
}

}  // namespace

}  // namespace gymnet
