// tools/launch_floor_probe.hip — what the kernel-argument round trip costs on the launch floor of the one-step kernels.
//
// Every step kernel takes its arguments as ONE struct by value (StepArgsT, ~250 bytes in the kernarg segment), so every wave begins
// with scalar loads from that segment and waits for them before it can issue its first vector load.  gfx950 can deliver the first
// kernel-argument words in user SGPRs at wave launch (-mllvm -amdgpu-kernarg-preload-count=N), but only for FLAT leading arguments:
// a struct passed by value is never preloaded.  This probe prices the round trip before the product's kernels change:
//   (a) empty        an empty kernel: the launch itself
//   (b) struct       the read-only half of the CartPole step — four state rows and the action, 16-byte non-temporal loads, four lanes
//                    per thread, the tick word — with its arguments in a by-value StepArgs; the loads are folded into one store per wave
//   (c) flat+preload the same body, the seven first-use words as flat leading arguments and the rest in a trailing StepArgs, compiled
//                    WITH the preload flag (this file compiled a second time with -DLAUNCH_FLOOR_PRELOAD_UNIT: tools/build_probes.sh)
//   (d) flat         (c)'s source compiled WITHOUT the flag: what the flattening alone does
//   (e) flat+preload, no scalar load before the first vector load: (c) still reads the workgroup size (a HIDDEN kernel argument, never
//                    preloaded while a by-value struct trails the flat ones) and the tick's parity from the kernarg segment, so its
//                    first vector load still waits for a scalar round trip.  (e) takes both as flat words — state, action, n,
//                    state_stride, tick2, reward, int32 block, int32 parity: 14 dwords — and is what "no round trip" really costs
// `launches` back-to-back launches per variant on one stream between two events, the variants interleaved, `rounds` times over.
// Not part of the product: built by tools/build_probes.sh into tools/build/.
//
//   usage: launch_floor_probe [launches = 2000] [rounds = 5]         (2^18 and 2^20 lanes)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>

#include "../gym.net_amd/csrc/kernels.hpp"
#include "../gym.net_amd/csrc/lanes.hpp"

using namespace gymnet;

// the read-only half of step_kernel<CartPole,4,true,false,15,*>: what one thread reads for its four lanes before it can advance them
__device__ __forceinline__ void read_half(const float *state, int64_t state_stride, const void *action, const uint64_t *tick2, int32_t parity,
                                          float *out, int64_t bdim) {
    const int64_t i0 = ((int64_t)blockIdx.x * bdim + threadIdx.x) * 4;
    const uint64_t tick = tick2[parity];
    float s[4][4];
    int32_t act[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) load_row<float, 4, true, false>(state + k * state_stride, i0, 0, s[k]);
    load_i32<4, true, false>(static_cast<const int32_t *>(action), i0, 0, act);
    uint32_t fold = (uint32_t)tick;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) fold ^= __float_as_uint(s[k][j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) fold ^= (uint32_t)act[j];
    // every lane's loads feed ONE word per wave
    const uint64_t m = __ballot(fold == 0x9E3779B9u);
    if (lane_id() == 0) out[i0 >> 8] = (float)__popcll(m);
}

#ifndef LAUNCH_FLOOR_PRELOAD_UNIT
__global__ __launch_bounds__(256) void floor_empty() {}

__global__ __launch_bounds__(256) void floor_struct(const StepArgs a) {
    if (((int64_t)blockIdx.x + 1) * blockDim.x * 4 > a.n) return;
    read_half(a.state, a.state_stride, a.action, a.tick2, a.parity, a.reward, blockDim.x);
}
#define FLAT_KERNEL floor_flat
#else
#define FLAT_KERNEL floor_flat_preload
#endif

__global__ __launch_bounds__(256) void FLAT_KERNEL(float *state, const void *action, int64_t n, int64_t state_stride, uint64_t *tick2,
                                                   float *reward, uint8_t *done, const StepArgs rest) {
    if (((int64_t)blockIdx.x + 1) * blockDim.x * 4 > n) return;
    read_half(state, state_stride, action, tick2, rest.parity, reward, blockDim.x);
}

void launch_flat_preload(const StepArgs &a, dim3 grid, hipStream_t st);
void launch_flat_preload_all(const StepArgs &a, dim3 grid, hipStream_t st);

#ifdef LAUNCH_FLOOR_PRELOAD_UNIT
__global__ __launch_bounds__(256) void floor_flat_preload_all(float *state, const void *action, int64_t n, int64_t state_stride, uint64_t *tick2,
                                                              float *reward, int32_t block, int32_t parity, const StepArgs rest) {
    if (((int64_t)blockIdx.x + 1) * block * 4 > n) return;
    read_half(state, state_stride, action, tick2, parity, reward, block);
}
void launch_flat_preload_all(const StepArgs &a, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL(floor_flat_preload_all, grid, dim3(256), 0, st, a.state, a.action, a.n, a.state_stride, a.tick2, a.reward, 256, a.parity, a);
}
void launch_flat_preload(const StepArgs &a, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL(floor_flat_preload, grid, dim3(256), 0, st, a.state, a.action, a.n, a.state_stride, a.tick2, a.reward, a.done, a);
}
#else

#define HIP_OK(x)                                                                                              \
    do {                                                                                                       \
        hipError_t e_ = (x);                                                                                   \
        if (e_ != hipSuccess) { std::fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); std::exit(2); } \
    } while (0)

constexpr int kVariants = 5;
static const char *kNames[kVariants] = {"(a) empty", "(b) struct", "(c) flat+preload", "(d) flat", "(e) preload, no s_load"};

int main(int argc, char **argv) {
    const int launches = argc > 1 ? std::atoi(argv[1]) : 2000;
    const int rounds = argc > 2 ? std::atoi(argv[2]) : 5;
    hipStream_t st;
    HIP_OK(hipStreamCreate(&st));
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0));
    HIP_OK(hipEventCreate(&e1));
    std::printf("# launch_floor_probe: %d back-to-back launches per variant on one stream, variants interleaved, %d rounds; us per launch\n",
                launches, rounds);
    for (const int64_t n : {(int64_t)1 << 18, (int64_t)1 << 20}) {
        float *state = nullptr, *reward = nullptr;
        int32_t *action = nullptr;
        uint8_t *done = nullptr;
        uint64_t *tick2 = nullptr;
        HIP_OK(hipMalloc(&state, (size_t)n * 4 * sizeof(float)));
        HIP_OK(hipMalloc(&reward, (size_t)n * sizeof(float)));
        HIP_OK(hipMalloc(&action, (size_t)n * sizeof(int32_t)));
        HIP_OK(hipMalloc(&done, (size_t)n));
        HIP_OK(hipMalloc(&tick2, 2 * sizeof(uint64_t)));
        HIP_OK(hipMemset(state, 0, (size_t)n * 4 * sizeof(float)));
        HIP_OK(hipMemset(action, 0, (size_t)n * sizeof(int32_t)));
        HIP_OK(hipMemset(tick2, 0, 2 * sizeof(uint64_t)));
        StepArgs a{};
        a.state = state; a.state_out = state; a.action = action; a.reward = reward; a.done = done; a.tick2 = tick2;
        a.n = n; a.state_stride = n;
        const dim3 grid((unsigned)(n / (4 * 256))), block(256);
        auto launch = [&](int v) {
            switch (v) {
            case 0: hipLaunchKernelGGL(floor_empty, grid, block, 0, st); break;
            case 1: hipLaunchKernelGGL(floor_struct, grid, block, 0, st, a); break;
            case 2: launch_flat_preload(a, grid, st); break;
            case 4: launch_flat_preload_all(a, grid, st); break;
            default: hipLaunchKernelGGL(floor_flat, grid, block, 0, st, a.state, a.action, a.n, a.state_stride, a.tick2, a.reward, a.done, a); break;
            }
        };
        std::vector<double> us[kVariants];
        for (int r = -1; r < rounds; ++r) {                      // round -1: warm-up, not recorded
            for (int v = 0; v < kVariants; ++v) {
                HIP_OK(hipEventRecord(e0, st));
                for (int l = 0; l < launches; ++l) launch(v);
                HIP_OK(hipEventRecord(e1, st));
                HIP_OK(hipEventSynchronize(e1));
                HIP_OK(hipGetLastError());
                float ms = 0.0f;
                HIP_OK(hipEventElapsedTime(&ms, e0, e1));
                if (r >= 0) us[v].push_back((double)ms * 1000.0 / launches);
            }
        }
        std::printf("lanes %lld\n", (long long)n);
        for (int v = 0; v < kVariants; ++v) {
            std::vector<double> s = us[v];
            std::sort(s.begin(), s.end());
            std::printf("  %-24s median %7.3f  min %7.3f  max %7.3f  range %6.3f   rounds:", kNames[v], s[s.size() / 2], s.front(), s.back(),
                        s.back() - s.front());
            for (double x : us[v]) std::printf(" %.3f", x);
            std::printf("\n");
        }
        std::fflush(stdout);
        HIP_OK(hipFree(state)); HIP_OK(hipFree(reward)); HIP_OK(hipFree(action)); HIP_OK(hipFree(done)); HIP_OK(hipFree(tick2));
    }
    return 0;
}
#endif
