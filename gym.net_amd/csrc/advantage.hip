// advantage.hip — generalized advantage estimation and discounted returns over the rows a rollout recorded.  The contract, operation for
// operation, is gymnet_gae_device in include/gymnet_amd.h; tests/_advantage_twin.py restates it in C and the GPU tests compare bits.
//
// One thread owns V consecutive lanes (columns) and walks t = T-1 .. 0 carrying A and vnext in registers: the recursion is serial in t
// and independent across lanes, so the kernel is a pure stream — every input element is read once (v[t+1] is the register vnext, never
// a second load), every output element written once.  The loads do not depend on the carried values, so the rows t-1 .. t-U are kept in
// flight in registers while row t is computed (a ring of U row buffers, statically indexed: the loops over it are fully unrolled).  The
// main loop runs while all U loads of a round are in range; the rows that remain, and any T < 2U, run the same round with wave-uniform
// guards.  Every thread reads row t of its own columns before it writes row t, and no pointer is __restrict__: an output may be the
// reward or the value array (the in-place forms of the header).
//
// V = 4 / V = 1 and whether values / boot exist are chosen by pick_advantage_form (advantage.hpp) and are template parameters; whether an
// output is NULL is a wave-uniform branch.  U and the cache hint are compile-time constants per V, the measured winners where each V runs
// (tools/advantage_probe.py, profiles/advantage_probe.txt, docs/ledger.md §advantage):
//   V = 4 (2^18 lanes and more): U = 4, non-temporal loads and stores.  At 2^20 x 256 over four visits to an MI355X: without values
//         (2.4 GB) non-temporal is 10 % faster every time; in place 5 % and 12 % faster in the two visits that timed it; out of place with
//         values (4.6 GB) from 7 % faster to 5 % slower, inside the 15 % by which the visits differ from each other.  Loads only or stores
//         only are never ahead of both.  U = 2, 4, 8 time the same with values; without them U = 8 is 5 % slower than U = 4;
//   V = 1 (fewer lanes, or a layout V = 4 cannot take): U = 8, plain accesses — with few waves the bytes each thread keeps in flight are
//         what fills the memory system (2^14 x 2048: 320 us at U = 8, 450 at U = 4, 660 at U = 2), and 4-byte non-temporal accesses are
//         3 % to 25 % slower than plain ones at 2^20 lanes.
// The probe rebuilds the unit with -DGYMNET_ADVANTAGE_U / -DGYMNET_ADVANTAGE_NT (both V alike) and -DGYMNET_ADVANTAGE_NARROW_BELOW=0 to
// time every candidate.
#include "advantage.hpp"
#include "handle.hpp"

#ifndef GYMNET_ADVANTAGE_NARROW_BELOW
#define GYMNET_ADVANTAGE_NARROW_BELOW ::gymnet::kAdvantageNarrowBelow
#endif

namespace gymnet {

namespace {

// rows in flight and the cache hint, per V
template <int V>
struct Tuning {
#ifdef GYMNET_ADVANTAGE_U
    static constexpr int U = GYMNET_ADVANTAGE_U;
#else
    static constexpr int U = V == 4 ? 4 : 8;
#endif
#ifdef GYMNET_ADVANTAGE_NT
    static constexpr int NT = GYMNET_ADVANTAGE_NT;         // bit 0: non-temporal loads, bit 1: non-temporal stores
#else
    static constexpr int NT = V == 4 ? 3 : 0;
#endif
    static constexpr bool NT_LOAD = (NT & 1) != 0, NT_STORE = (NT & 2) != 0;
    static_assert(U == 2 || U == 4 || U == 8, "rows in flight: 2, 4 or 8");
};

struct AdvantageArgs {
    const float *reward; const uint8_t *done; const float *value; const float *last_value; const float *boot;
    float *advantage; float *ret;
    int64_t steps, threads, stride;
    float gamma, gl;                                        // gl = gamma * lambda, one float32 product formed on the host
};

typedef float float4v __attribute__((ext_vector_type(4)));

template <int V> struct Wide;
template <> struct Wide<1> { using F = float; using D = uint8_t; };
template <> struct Wide<4> { using F = float4v; using D = uint32_t; };

template <bool NT, class T>
__device__ __forceinline__ T load_once(const T *p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
template <bool NT, class T>
__device__ __forceinline__ void store_once(T *p, T v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

__device__ __forceinline__ float lane_of(float v, int) { return v; }
__device__ __forceinline__ float lane_of(float4v v, int j) { return v[j]; }
__device__ __forceinline__ void set_lane(float &v, int, float x) { v = x; }
__device__ __forceinline__ void set_lane(float4v &v, int j, float x) { v[j] = x; }

template <int V, bool HAS_V, bool HAS_B>
struct AdvRow {
    typename Wide<V>::F r, v, b;
    typename Wide<V>::D d;
    // row t of the thread's columns, first column `col`
    __device__ __forceinline__ void load(const AdvantageArgs &a, int64_t t, int64_t col) {
        const int64_t off = t * a.stride + col;
        r = load_once<Tuning<V>::NT_LOAD>(reinterpret_cast<const typename Wide<V>::F *>(a.reward + off));
        d = load_once<Tuning<V>::NT_LOAD>(reinterpret_cast<const typename Wide<V>::D *>(a.done + off));
        if constexpr (HAS_V) v = load_once<Tuning<V>::NT_LOAD>(reinterpret_cast<const typename Wide<V>::F *>(a.value + off));
        if constexpr (HAS_B) b = load_once<Tuning<V>::NT_LOAD>(reinterpret_cast<const typename Wide<V>::F *>(a.boot + off));
    }
};

template <int V, bool HAS_V, bool HAS_B>
__device__ __forceinline__ void advantage_row(const AdvantageArgs &a, const AdvRow<V, HAS_V, HAS_B> &row, int64_t t, int64_t col,
                                              float (&A)[V], float (&vnext)[V]) {
    typename Wide<V>::F adv, ret;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const uint32_t d = ((uint32_t)row.d >> (8 * j)) & 0xFFu;
        const float r = lane_of(row.r, j);
        const float v = HAS_V ? lane_of(row.v, j) : 0.0f;
        const float boot = HAS_B ? lane_of(row.b, j) : 0.0f;
        const float nv = (d & 1u) ? 0.0f : (d & 2u) ? boot : vnext[j];               // terminated wins over truncated
        const float delta = __builtin_fmaf(a.gamma, nv, r) - v;
        A[j] = d != 0u ? delta : __builtin_fmaf(a.gl, A[j], delta);
        set_lane(adv, j, A[j]);
        set_lane(ret, j, A[j] + v);
        vnext[j] = v;
    }
    const int64_t off = t * a.stride + col;
    if (a.advantage) store_once<Tuning<V>::NT_STORE>(reinterpret_cast<typename Wide<V>::F *>(a.advantage + off), adv);     // wave-uniform
    if (a.ret) store_once<Tuning<V>::NT_STORE>(reinterpret_cast<typename Wide<V>::F *>(a.ret + off), ret);
}

template <int V, bool HAS_V, bool HAS_B>
__global__ __launch_bounds__(kAdvantageBlock) void advantage_kernel(const AdvantageArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.threads) return;                              // the tail is guarded, nothing is padded: V = 4 only where count % 4 == 0
    const int64_t col = i * V;
    float A[V], vnext[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { A[j] = 0.0f; vnext[j] = 0.0f; }
    if (a.last_value) {                                      // wave-uniform
        const typename Wide<V>::F lv = *reinterpret_cast<const typename Wide<V>::F *>(a.last_value + col);
#pragma unroll
        for (int j = 0; j < V; ++j) vnext[j] = lane_of(lv, j);
    }
    constexpr int kU = Tuning<V>::U;
    AdvRow<V, HAS_V, HAS_B> ring[kU];                        // ring[k] holds row t - k at the head of a round
    int64_t t = a.steps - 1;
#pragma unroll
    for (int k = 0; k < kU; ++k)
        if (t - k >= 0) ring[k].load(a, t - k, col);
    for (; t >= 2 * kU - 1; t -= kU) {                       // every load of the round is in range: t - (kU - 1) - kU >= 0
#pragma unroll
        for (int k = 0; k < kU; ++k) {
            advantage_row<V, HAS_V, HAS_B>(a, ring[k], t - k, col, A, vnext);
            ring[k].load(a, t - k - kU, col);
        }
    }
    for (; t >= 0; t -= kU) {                                // the guarded epilogue: the last rows, and every row where T < 2U
#pragma unroll
        for (int k = 0; k < kU; ++k) {
            if (t - k >= 0) {
                advantage_row<V, HAS_V, HAS_B>(a, ring[k], t - k, col, A, vnext);
                if (t - k - kU >= 0) ring[k].load(a, t - k - kU, col);
            }
        }
    }
}

template <int V>
hipError_t launch_advantage_vec(const AdvantageForm &f, const AdvantageArgs &a, hipStream_t st) {
    const dim3 grid((unsigned)f.blocks), block(kAdvantageBlock);
    if (f.has_value) {
        if (f.has_boot) hipLaunchKernelGGL((advantage_kernel<V, true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((advantage_kernel<V, true, false>), grid, block, 0, st, a);
    } else {
        if (f.has_boot) hipLaunchKernelGGL((advantage_kernel<V, false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((advantage_kernel<V, false, false>), grid, block, 0, st, a);
    }
    return hipGetLastError();
}

hipError_t launch_advantage(const AdvantageForm &f, const AdvantageArgs &a, hipStream_t st) {
    return f.vec == 4 ? launch_advantage_vec<4>(f, a, st) : launch_advantage_vec<1>(f, a, st);
}

}  // namespace

}  // namespace gymnet

using namespace gymnet;

extern "C" {

int gymnet_gae_device(int device, void *stream, int64_t steps, int64_t count, int64_t stride, const float *d_reward, const uint8_t *d_done,
                      const float *d_value, const float *d_last_value, const float *d_boot, float gamma, float lambda, float *d_advantage,
                      float *d_return) {
    return guarded([&]() -> int {
    if (steps < 0 || count < 0 || stride < 0) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "gae: steps %lld, count %lld and stride %lld must be >= 0", (long long)steps, (long long)count, (long long)stride);
    if (stride < count) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "gae: stride %lld < count %lld", (long long)stride, (long long)count);
    if (!(__builtin_isfinite(gamma) && gamma >= 0.0f && gamma <= 1.0f)) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "gae: gamma must be finite and in [0, 1]");
    if (!(__builtin_isfinite(lambda) && lambda >= 0.0f && lambda <= 1.0f)) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "gae: lambda must be finite and in [0, 1]");
    if (!d_advantage && !d_return) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "gae: d_advantage and d_return are both null");
    if (!d_reward || !d_done) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "gae: d_reward / d_done is null");
    // an output may be the reward or the value array (each element is read before it is written: the in-place forms); nothing else may alias
    if (d_advantage == d_return) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "gae: d_advantage and d_return are the same array");
    for (const float *out : {d_advantage, d_return}) {
        if (!out) continue;
        if ((const void *)out == (const void *)d_done || out == d_boot || out == d_last_value)
            return fail(nullptr, GYMNET_ERR_INVALID_ARG, "gae: an output may alias d_reward or d_value only, not d_done / d_boot / d_last_value");
    }
    for (const void *p : {(const void *)d_reward, (const void *)d_value, (const void *)d_last_value, (const void *)d_boot, (const void *)d_advantage, (const void *)d_return})
        if (((uintptr_t)p & 3u) != 0) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "gae: float arrays must be 4-byte aligned");
    if (steps == 0 || count == 0) return GYMNET_OK;
    if (steps > 1 && stride > INT64_MAX / 4 / steps) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "gae: steps x stride overflows");
    const AdvantagePointers ptrs{(uintptr_t)d_reward, (uintptr_t)d_done, (uintptr_t)d_value, (uintptr_t)d_last_value, (uintptr_t)d_boot,
                                 (uintptr_t)d_advantage, (uintptr_t)d_return};
    const AdvantageForm f = pick_advantage_form(count, stride, ptrs, GYMNET_ADVANTAGE_NARROW_BELOW);
    if (f.blocks > 0x7FFFFFFF) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "gae: count %lld is beyond one launch's grid", (long long)count);
    const AdvantageArgs a{d_reward, d_done, d_value, d_last_value, d_boot, d_advantage, d_return, steps, f.threads, stride, gamma, gamma * lambda};
    DeviceScope scope;
    (void)hipGetLastError();
    HIP_TRY(nullptr, hipSetDevice(device));
    HIP_TRY(nullptr, launch_advantage(f, a, static_cast<hipStream_t>(stream)));
    return GYMNET_OK;
    });
}

}  // extern "C"
