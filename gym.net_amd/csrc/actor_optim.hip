// actor_optim.hip — one update of one flat parameter vector from its gradient: the step that follows actor_grad.hip's gradient, so that a
// host without torch can train without a trip to the host.  The contract and the arithmetic, rule for rule, are
// gymnet_vecenv_actor_apply_gradient's in include/gymnet_amd.h; what a call is refused for and the scalars it is given are actor_optim.hpp.
//
// At most 8192 parameters: 32 KB each of weights and gradient and 64 KB of state.  The call is bound by latency, not by bandwidth, so what
// it must not pay is a second launch or a second pass over memory for the norm that clipping needs before the first weight can change.
//   work split   ONE workgroup of 1024 threads (sixteen waves, four a SIMD of one CU), one launch.  Thread i owns the elements i, i + 1024,
//                .. i + 7 * 1024: every load and store instruction of a wave covers 64 consecutive floats, and nothing is asked of the
//                caller's pointers beyond a float's alignment (a torch view into a flat tensor starts anywhere).
//   loads        a thread's weights, gradients and state elements — up to 32 dwords — are all requested before the first use of any:
//                the unrolled element loop has no dependence between its iterations, and the one wait of the kernel sits behind the last
//                request.  Elements at or past count are never requested and take the value +0.
//   norm         from the gradients already in registers, in a fixed order: per thread in float64 over its elements in ascending order;
//                across the wave by six __shfl_xor steps (1, 2, .. 32: both partners add the same two values, so all 64 lanes hold the
//                same bits); the sixteen wave sums through 128 bytes of LDS, added in wave order by EVERY thread after the kernel's one
//                barrier, so each thread forms the same norm and the same coef itself and nothing is broadcast.  No atomics: the same
//                inputs give the same bits.  A call that neither clips nor wants the norm skips the reduction and the barrier (a uniform
//                branch: a second template flag would double the instantiations to save one scalar compare).
//   update       float32, every operation rounding on its own (-ffp-contract=off; / and sqrtf correctly rounded), templated on the rule:
//                three instantiations.  SGD without momentum (a null state) neither loads nor stores a state row, decided by a uniform
//                branch.  Stores are plain vector stores of live elements only.
// Nothing is read twice and nothing is written that the rule does not change (d_grad is read only).
//
// Out of scope: a joint norm over several vectors, AdamW's decoupled decay, Nesterov, amsgrad, schedules, optimiser state in the handle,
// an epoch or minibatch loop, fusing the step into actor_grad_reduce_kernel, float64 parameters.
#include "actor_optim.hpp"
#include "actor_net.hpp"

namespace gymnet {

static_assert(kOptimMaxParams == kActorMaxParams, "actor_net.hpp's limit");
static_assert(kOptimSgd == GYMNET_OPT_SGD && kOptimAdadelta == GYMNET_OPT_ADADELTA && kOptimAdam == GYMNET_OPT_ADAM, "the header's rule numbers");

namespace {

constexpr int kWaves = kOptimThreads / 64;

struct OptimArgs {
    float *w;
    const float *g;
    float *s0, *s1;                               // the state rows; both null: SGD without momentum
    float *norm;                                  // null: not wanted
    int32_t count;
    int32_t reduce;                               // the norm is needed: to clip, or to report
    float max_norm;                               // 0: no clipping
    OptimScalars k;
};

template <int RULE>
__global__ __launch_bounds__(kOptimThreads) void actor_optim_kernel(const OptimArgs a) {
    constexpr int E = kOptimPerThread;
    constexpr bool kRow1 = RULE != kOptimSgd;     // AdaDelta and Adam keep two state rows
    const int tid = (int)threadIdx.x;
    const bool row0 = a.s0 != nullptr;            // uniform; always true for AdaDelta and Adam (actor_optim_refusal)
    float w[E], g[E], s0[E], s1[E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int i = tid + j * kOptimThreads;
        const bool live = i < a.count;
        w[j] = live ? a.w[i] : 0.0f;
        g[j] = live ? a.g[i] : 0.0f;
        s0[j] = live && row0 ? a.s0[i] : 0.0f;
        s1[j] = live && kRow1 ? a.s1[i] : 0.0f;
    }
    float coef = 1.0f;
    if (a.reduce) {
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < E; ++j) sum += (double)g[j] * (double)g[j];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) sum += __shfl_xor(sum, o, 64);
        __shared__ double wave_sum[kWaves];
        if ((tid & 63) == 0) wave_sum[tid >> 6] = sum;
        __syncthreads();
        double total = 0.0;
#pragma unroll
        for (int v = 0; v < kWaves; ++v) total += wave_sum[v];
        const double norm = sqrt(total);
        if (a.norm && tid == 0) *a.norm = (float)norm;
        if (a.max_norm > 0.0f) {
            const double c = (double)a.max_norm / (norm + 1e-6);
            coef = (float)(c > 1.0 ? 1.0 : c);    // (a NaN norm stays a NaN coef, as torch's clamp keeps it)
        }
    }
    const OptimScalars k = a.k;
    const bool clip = a.max_norm > 0.0f, decay = k.weight_decay != 0.0f;
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int i = tid + j * kOptimThreads;
        if (i >= a.count) continue;
        float gj = g[j];
        if (clip) gj = gj * coef;
        if (decay) gj = gj + k.weight_decay * w[j];
        if constexpr (RULE == kOptimSgd) {
            const float b = k.p0 * s0[j] + gj;
            a.w[i] = w[j] - k.lr * b;
            if (row0) a.s0[i] = b;
        } else if constexpr (RULE == kOptimAdadelta) {
            const float q = k.p0 * s0[j] + k.q0 * (gj * gj);
            const float d = sqrtf(s1[j] + k.eps) / sqrtf(q + k.eps) * gj;
            a.w[i] = w[j] - k.lr * d;
            a.s0[i] = q;
            a.s1[i] = k.p0 * s1[j] + k.q0 * (d * d);
        } else {
            const float m = k.p0 * s0[j] + k.q0 * gj;
            const float v = k.p1 * s1[j] + k.q1 * (gj * gj);
            a.w[i] = w[j] - k.lr * (m / (sqrtf(v) / k.bias2 + k.eps));
            a.s0[i] = m;
            a.s1[i] = v;
        }
    }
}

}  // namespace

}  // namespace gymnet

using namespace gymnet;

extern "C" {

int gymnet_vecenv_actor_apply_gradient(gymnet_vecenv *h, int32_t rule, float *d_weights, int64_t count, const float *d_grad, float *d_state,
                                       int64_t step, float lr, float p0, float p1, float eps, float weight_decay, float max_grad_norm,
                                       float *d_norm) {
    return guarded([&]() -> int {
    ENTER(h);
    const ActorOptimCall c{rule, (uintptr_t)d_weights, (uintptr_t)d_grad, (uintptr_t)d_state, (uintptr_t)d_norm, count, step,
                           lr, p0, p1, eps, weight_decay, max_grad_norm};
    if (const char *why = actor_optim_refusal(c)) return fail(h, GYMNET_ERR_INVALID_ARG, "actor_apply_gradient: %s", why);
    OptimArgs a{};
    a.w = d_weights; a.g = d_grad; a.norm = d_norm;
    if (optim_uses_state(rule, p0)) {
        a.s0 = d_state;
        a.s1 = d_state + count;
    }
    a.count = (int32_t)count;
    a.max_norm = max_grad_norm;
    a.reduce = max_grad_norm > 0.0f || d_norm != nullptr;
    a.k = optim_scalars(c);
    const dim3 grid(1), block(kOptimThreads);
    if (rule == kOptimSgd) hipLaunchKernelGGL(actor_optim_kernel<kOptimSgd>, grid, block, 0, h->stream, a);
    else if (rule == kOptimAdadelta) hipLaunchKernelGGL(actor_optim_kernel<kOptimAdadelta>, grid, block, 0, h->stream, a);
    else hipLaunchKernelGGL(actor_optim_kernel<kOptimAdam>, grid, block, 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
    return GYMNET_OK;
    });
}

}  // extern "C"
