// actor_grad.hip — the gradient of a minibatch loss with respect to an actor's or a critic's flat weights: the one dense contraction on
// the library's hot path, and so its one use of the matrix cores.  The contract, loss for loss, is gymnet_vecenv_actor_policy_gradient /
// gymnet_vecenv_actor_value_gradient in include/gymnet_amd.h; what a call is refused for and how its launch is sized is actor_grad.hpp.
//
// The network (at most 4 layers, widths <= 64, <= 8192 parameters) fits in LDS whole, so a workgroup keeps it there and walks row tiles:
//   work split   256 threads = four waves; G = min(ceil(m / 16), kGradBlocks) workgroups; block b takes the tiles b, b + G, .. of R = 16
//                rows.  R = 32 does not fit: weights at their pitch (<= 37.9 KB) plus 4 + 1 activation-sized tiles of 32 x 68 floats are
//                81 KB; at R = 16 the kernel holds 64 832 bytes of static LDS and two workgroups share a CU.
//   staging      on entry a block copies the caller's flat W_l [out][in] into LDS at pitch grad_pitch(in) (actor_grad.hpp: why every
//                operand read below is free of bank conflicts) and keeps its four bias values per lane in registers.
//   forward      A_{l+1} = relu(A_l W_l^T + b_l) on v_mfma_f32_16x16x4_f32: M = the tile's 16 rows, N = 16 outputs, K = the inputs 4 at
//                a time; the <= 4 output tiles of a layer go to the four waves; the accumulator starts as the bias.  Every A_l stays in
//                LDS for the backward pass; the last layer's values land in the dZ tile.
//   head         one thread per row, plain float32 (exp_neg.hpp, log_pos.hpp): the row's logp / value, its loss term, and dZ_L unscaled
//                into LDS, as [row][out] and transposed [out][row].
//   backward     last layer to first: dW_l += dZ_l^T A_l (M = outputs, N = inputs, K = the 16 rows: four instructions a tile) into
//                accumulators that stay in registers across all of the block's tiles — at most 16 tiles a layer, tile q of a layer with
//                wave q % 4 in slot q / 4; db_l as column sums by wave 0; dA_l = dZ_l W_l (M = rows, N = inputs, K = outputs) from the
//                transposed dZ, masked by A_l > 0 into dZ_{l-1}.
//   reduction    each block writes its partial gradient and loss once, to scratch [b][count + 1]; actor_grad_reduce_kernel sums the G
//                partials of a parameter in block order (in a double, rounded once), divides by m and writes d_grad / d_loss.  No
//                atomics: the same inputs give the same bits.
// The FP32 MFMA keeps float32 products and sums (no reduced-precision type anywhere), but sums in another order than actor_forward's fmaf
// chain: logp / value agree with the rollout's records to rounding, not bit for bit.
//
// Out of scope: the Box actor's Gaussian log-density gradient (tanh head), PPO value clipping, a trunk shared between actor and critic,
// gradients accumulated across calls, the optimiser step, fusing the rows= gather of gymnet_rollout_inputs_device into this kernel, float64
// networks.
#include "actor_grad.hpp"
#include "actor_net.hpp"
#include "exp_neg.hpp"
#include "log_pos.hpp"

namespace gymnet {

static_assert(kGradMaxLayers == kActorMaxLayers && kGradMaxWidth == kActorMaxWidth && kGradMaxParams == kActorMaxParams, "actor_net.hpp's limits");

namespace {

constexpr int kR = kGradRows, kP = kGradPitch, kPT = kGradPitchT, kL = kGradMaxLayers;

typedef float floatx4 __attribute__((ext_vector_type(4)));

struct GradArgs {
    GradNet net;
    const float *w, *x;
    int64_t x_stride, m, tiles;
    const int32_t *actions;                       // policy
    const float *aux;                             // policy: coef; value: target
    const float *logp_old;                        // policy, or null
    float clip, entropy_coef, inv_tau;
    int32_t action_n;
    float *scratch;                               // [blocks][count + 1]
    float *row_out;                               // logp / value [m], or null
};

// D += A B for A [16][4], B [4][16], D [16][16]: lane (i, k) = (lane % 16, lane / 16) gives A[i][k] and B[k][i], and holds D[4 * k + r][i] in d[r]
__device__ __forceinline__ floatx4 mfma(float a, float b, floatx4 d) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, d, 0, 0, 0); }

// exp(d) for either sign from exp_neg
__device__ __forceinline__ float exp_any(float d) { return d <= 0.0f ? exp_neg(d) : 1.0f / exp_neg(-d); }

// one row of the policy loss: z -> dz (both [16], zeros beyond action_n), the row's loss term -(s + entropy_coef * H), its logp
__device__ __forceinline__ float policy_row(const GradArgs &a, int64_t row, float (&z)[16], float &logp) {
    const int32_t n = a.action_n;
    float zmax = z[0];
#pragma unroll
    for (int k = 1; k < kActorMaxActions; ++k) if (k < n && z[k] > zmax) zmax = z[k];
    float s[kActorMaxActions], e[kActorMaxActions];
    float run = 0.0f;
#pragma unroll
    for (int k = 0; k < kActorMaxActions; ++k) {
        s[k] = 0.0f; e[k] = 0.0f;
        if (k < n) {                                                         // wave-uniform
            s[k] = (z[k] - zmax) * a.inv_tau;
            e[k] = exp_neg(s[k]);
            run = run + e[k];
        }
    }
    const float lse = log_pos(run);
    const float inv_run = 1.0f / run;
    const int32_t act = a.actions[row];
    const bool bad = act < 0 || act >= n;                                    // never an index: selected by compare below
    float sa = 0.0f;
#pragma unroll
    for (int k = 0; k < kActorMaxActions; ++k) sa = k == act ? s[k] : sa;
    const float nan = __builtin_bit_cast(float, 0x7FC00000u);
    logp = bad ? nan : sa - lse;
    float ent = 0.0f;
#pragma unroll
    for (int k = 0; k < kActorMaxActions; ++k) {
        if (k < n) ent = ent - (e[k] * inv_run) * (s[k] - lse);
    }
    const float coef = a.aux[row];
    float obj, g;                                                            // the row's objective s_i and d s_i / d logp
    if (a.logp_old) {                                                        // wave-uniform
        const float r = exp_any(logp - a.logp_old[row]);
        const float lo = 1.0f - a.clip, hi = 1.0f + a.clip;
        const float rc = r < lo ? lo : (r > hi ? hi : r);
        const float u = r * coef, c = rc * coef;
        const bool unclipped = u <= c;                                       // ties go to the unclipped term
        obj = unclipped ? u : c;
        g = unclipped ? u : 0.0f;
    } else {
        obj = coef * logp;
        g = coef;
    }
    if (bad) { obj = nan; g = nan; }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        float dz = 0.0f;
        if (k < kActorMaxActions && k < n) {
            const float p = e[k] * inv_run;
            const float lpk = s[k] - lse;
            const float dobj = g * ((k == act ? 1.0f : 0.0f) - p) - a.entropy_coef * (p * (lpk + ent));
            dz = -(dobj * a.inv_tau);
        }
        z[k] = dz;
    }
    return -(obj + a.entropy_coef * ent);
}

template <bool POLICY>
__global__ __launch_bounds__(256) void actor_grad_kernel(const GradArgs a) {
    __shared__ float sW[kGradLdsWeights];
    __shared__ float sA[kL][kR * kP];
    __shared__ float sZ[kR * kP];                                            // the last layer's values, then dZ_l [row][out]
    __shared__ __attribute__((aligned(16))) float sZT[kGradMaxWidth * kPT];  // dZ_l [out][row]
    __shared__ float sLoss[kR];
    const GradNet &net = a.net;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = tid & 15, lk = (tid & 63) >> 4;

    // ---- staging: zeros everywhere an operand read may land, then the weights at their pitch
    for (int e = tid; e < kGradLdsWeights; e += 256) sW[e] = 0.0f;
    for (int e = tid; e < kL * kR * kP; e += 256) (&sA[0][0])[e] = 0.0f;
    for (int e = tid; e < kR * kP; e += 256) sZ[e] = 0.0f;
    for (int e = tid; e < kGradMaxWidth * kPT; e += 256) sZT[e] = 0.0f;
    __syncthreads();
    float bias[kL];
#pragma unroll
    for (int l = 0; l < kL; ++l) {
        bias[l] = 0.0f;
        if (l < net.layers) {                                                // wave-uniform
            const int32_t win = net.win[l], wout = net.wout[l];
            const float *wl = a.w + net.off[l];
            for (int e = tid; e < wout * win; e += 256) {
                const int o = e / win, j = e - o * win;
                sW[net.lds[l] + o * net.pitch[l] + j] = wl[e];
            }
            const int o = 16 * wave + li;
            if (o < wout) bias[l] = wl[wout * win + o];
        }
    }
    __syncthreads();

    floatx4 acc[kL][4];                                                      // dW_l tile q = wave + 4 * slot, across all of the block's tiles
#pragma unroll
    for (int l = 0; l < kL; ++l)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[l][s] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
    float db[kL] = {0.0f, 0.0f, 0.0f, 0.0f};                                 // wave 0: db_l[tid]
    float loss = 0.0f;                                                       // threads 0 .. 15: the loss terms of row tid of every tile

    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t row0 = tile * kR;
        // ---- A_0 = the tile of x, +0 beyond m and beyond win
#pragma unroll
        for (int q = 0; q < kR * kGradMaxWidth / 256; ++q) {
            const int e = tid + 256 * q, r = e >> 6, c = e & 63;
            const int64_t row = row0 + r;
            sA[0][r * kP + c] = (row < a.m && c < net.win[0]) ? a.x[row * a.x_stride + c] : 0.0f;
        }
        __syncthreads();
        // ---- forward
#pragma unroll
        for (int l = 0; l < kL; ++l) {
            if (l < net.layers) {                                            // wave-uniform
                const int32_t win = net.win[l], wout = net.wout[l];
                const bool hidden = l + 1 < net.layers;
                if (16 * wave < wout) {                                      // wave-uniform: output tile `wave`
                    const int o = 16 * wave + li;
                    const bool ok = o < wout;
                    const float *wrow = sW + net.lds[l] + (ok ? o : 0) * net.pitch[l] + lk;
                    const float *arow = sA[l] + li * kP + lk;
                    const int nch = (win + 3) >> 2;
                    floatx4 z = floatx4{bias[l], bias[l], bias[l], bias[l]};
#pragma unroll
                    for (int c = 0; c < kGradMaxWidth / 4; ++c) {
                        if (c < nch) {                                       // wave-uniform
                            const float wv = wrow[4 * c];
                            z = mfma(arow[4 * c], ok ? wv : 0.0f, z);
                        }
                    }
                    float *dst = (hidden && l + 1 < kL) ? sA[(l + 1) & (kL - 1)] : sZ;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = z[r];
                        dst[(4 * lk + r) * kP + o] = hidden ? (v > 0.0f ? v : 0.0f) : v;
                    }
                }
                __syncthreads();
            }
        }
        // ---- head: one thread per row
        if (tid < kR) {
            const int64_t row = row0 + tid;
            float z[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) z[k] = 0.0f;
            if (row < a.m) {
                if constexpr (POLICY) {
#pragma unroll
                    for (int k = 0; k < kActorMaxActions; ++k) z[k] = sZ[tid * kP + k];
                    float logp;
                    loss = loss + policy_row(a, row, z, logp);
                    if (a.row_out) a.row_out[row] = logp;
                } else {
                    const float v = sZ[tid * kP];
                    const float d = v - a.aux[row];
                    loss = loss + 0.5f * (d * d);
                    z[0] = d;
                    if (a.row_out) a.row_out[row] = v;
                }
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) { sZ[tid * kP + k] = z[k]; sZT[k * kPT + tid] = z[k]; }
        }
        __syncthreads();
        // ---- backward, last layer to first
#pragma unroll
        for (int l = kL - 1; l >= 0; --l) {
            if (l < net.layers) {                                            // wave-uniform
                const int32_t win = net.win[l], wout = net.wout[l];
                const int To = (wout + 15) >> 4, Ti = (win + 15) >> 4;
                // dW_l += dZ_l^T A_l: K = the rows t, t + 4, t + 8, t + 12
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int q = wave + 4 * s;
                    if (q < To * Ti) {                                       // wave-uniform
                        const int ti = q / To, to = q - ti * To;
                        const float *zc = sZ + 4 * lk * kP + 16 * to + li;
                        const float *ac = sA[l] + 4 * lk * kP + 16 * ti + li;
#pragma unroll
                        for (int t = 0; t < 4; ++t) acc[l][s] = mfma(zc[t * kP], ac[t * kP], acc[l][s]);
                    }
                }
                if (wave == 0 && tid < wout) {
                    float sum = 0.0f;
#pragma unroll
                    for (int r = 0; r < kR; ++r) sum = sum + sZ[r * kP + tid];
                    db[l] = db[l] + sum;
                }
                // dA_l = dZ_l W_l for input tile `wave`, K = the outputs 16 * ob + t + 4 * k; masked by A_l > 0 (a product, so that a NaN stays)
                const bool back = l > 0 && 16 * wave < win;                  // wave-uniform
                const int j = 16 * wave + li;
                floatx4 d = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
                if (back) {
                    const bool okj = j < win;
#pragma unroll
                    for (int ob = 0; ob < 4; ++ob) {
                        if (ob < To) {                                       // wave-uniform
#pragma unroll
                            for (int t = 0; t < 4; ++t) {
                                const int o = 16 * ob + t + 4 * lk;
                                const bool ok = okj && o < wout;
                                const float wv = sW[net.lds[l] + (ok ? o * net.pitch[l] + j : 0)];
                                d = mfma(sZT[o * kPT + li], ok ? wv : 0.0f, d);
                            }
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) d[r] = d[r] * (sA[l][(4 * lk + r) * kP + j] > 0.0f ? 1.0f : 0.0f);
                }
                __syncthreads();                                             // every read of dZ_l is done
                if (back) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) sZ[(4 * lk + r) * kP + j] = d[r];
                    *reinterpret_cast<floatx4 *>(sZT + j * kPT + 4 * lk) = d;
                }
                __syncthreads();
            }
        }
    }

    // ---- the block's partial gradient and loss, once
    float *part = a.scratch + (int64_t)blockIdx.x * (net.count + 1);
#pragma unroll
    for (int l = 0; l < kL; ++l) {
        if (l < net.layers) {                                                // wave-uniform
            const int32_t win = net.win[l], wout = net.wout[l];
            const int To = (wout + 15) >> 4, Ti = (win + 15) >> 4;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int q = wave + 4 * s;
                if (q < To * Ti) {                                           // wave-uniform
                    const int ti = q / To, to = q - ti * To;
                    const int j = 16 * ti + li;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int o = 16 * to + 4 * lk + r;
                        if (o < wout && j < win) part[net.off[l] + o * win + j] = acc[l][s][r];
                    }
                }
            }
            if (wave == 0 && tid < wout) part[net.off[l] + wout * win + tid] = db[l];
        }
    }
    if (tid < kR) sLoss[tid] = loss;
    __syncthreads();
    if (tid == 0) {
        float sum = 0.0f;
#pragma unroll
        for (int r = 0; r < kR; ++r) sum = sum + sLoss[r];
        part[net.count] = sum;
    }
}

// parameter i (i == count: the loss): the blocks' partials in block order, over m.  The running sum is a double, rounded to float32 once at the
// end: up to 512 partials of either sign summed in float32 lose several units in the last place, more than torch's own float32 gradient
__global__ __launch_bounds__(256) void actor_grad_reduce_kernel(const float *__restrict__ scratch, int32_t blocks, int32_t count, double m,
                                                                float *__restrict__ grad, float *__restrict__ loss) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > count) return;
    double sum = 0.0;
    for (int b = 0; b < blocks; ++b) sum = sum + (double)scratch[(int64_t)b * (count + 1) + i];
    const float out = (float)(sum / m);
    if (i < count) grad[i] = out;
    else if (loss) *loss = out;
}

// the handle's scratch: kGradBlocks partials of the largest network, allocated on the first call and gone with the actor
int grad_scratch(gymnet_vecenv *h, float *&scratch) {
    Actor &ac = *h->actor;
    if (!ac.grad_scratch) {
        ac.grad_scratch = static_cast<float *>(ac.mem.take(sizeof(float) * (size_t)kGradBlocks * (kGradMaxParams + 1)));
        if (!ac.grad_scratch) return fail(h, GYMNET_ERR_OOM, "hipMalloc of the gradient scratch failed");
    }
    scratch = ac.grad_scratch;
    return GYMNET_OK;
}

int actor_gradient(gymnet_vecenv *h, bool policy, const float *d_weights, int64_t count, const float *d_x, int64_t x_stride, int64_t m,
                   const int32_t *d_actions, const float *d_aux, const float *d_logp_old, float clip, float entropy_coef, float *d_grad, float *d_loss,
                   float *d_row_out) {
    const Actor *ac = h->actor;
    const ActorNet *an = !ac ? nullptr : (policy ? &ac->net : &ac->critic);
    const bool has_net = an && an->layers > 0;
    const ActorGradCall c{policy, ac != nullptr, ac && ac->box, ac && ac->has_critic(), !ac ? 0 : (policy ? ac->count : ac->critic_count),
                          has_net ? an->win[0] : 0, count, x_stride, m, (uintptr_t)d_weights, (uintptr_t)d_x, (uintptr_t)d_actions, (uintptr_t)d_aux,
                          (uintptr_t)d_logp_old, (uintptr_t)d_grad, clip, entropy_coef};
    if (const char *why = actor_grad_refusal(c)) return fail(h, GYMNET_ERR_INVALID_ARG, "%s: %s", policy ? "actor_policy_gradient" : "actor_value_gradient", why);
    GradArgs a{};
    if (grad_net_shape(a.net, an->layers, an->win, an->wout) > kGradLdsWeights || a.net.count != count)
        return fail(h, GYMNET_ERR_HIP, "actor gradient: the network does not fit the kernel's LDS plan");
    const ActorGradForm f = pick_actor_grad_form(m);
    ST_TRY(grad_scratch(h, a.scratch));
    a.w = d_weights; a.x = d_x; a.x_stride = x_stride; a.m = m; a.tiles = f.tiles;
    a.actions = d_actions; a.aux = d_aux; a.logp_old = d_logp_old;
    a.clip = clip; a.entropy_coef = entropy_coef; a.inv_tau = ac->inv_tau; a.action_n = an->action_n;
    a.row_out = d_row_out;
    if (policy) hipLaunchKernelGGL(actor_grad_kernel<true>, dim3((unsigned)f.blocks), dim3(256), 0, h->stream, a);
    else hipLaunchKernelGGL(actor_grad_kernel<false>, dim3((unsigned)f.blocks), dim3(256), 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(actor_grad_reduce_kernel, dim3((unsigned)((count + 1 + 255) / 256)), dim3(256), 0, h->stream, a.scratch, f.blocks, (int32_t)count,
                       (double)m, d_grad, d_loss);
    HIP_TRY(h, hipGetLastError());
    return GYMNET_OK;
}

}  // namespace

}  // namespace gymnet

using namespace gymnet;

extern "C" {

int gymnet_vecenv_actor_policy_gradient(gymnet_vecenv *h, const float *d_weights, int64_t count, const float *d_x, int64_t x_stride, int64_t m,
                                        const int32_t *d_actions, const float *d_coef, const float *d_logp_old, float clip, float entropy_coef,
                                        float *d_grad, float *d_loss, float *d_logp) {
    return guarded([&]() -> int {
    ENTER(h);
    return actor_gradient(h, true, d_weights, count, d_x, x_stride, m, d_actions, d_coef, d_logp_old, clip, entropy_coef, d_grad, d_loss, d_logp);
    });
}

int gymnet_vecenv_actor_value_gradient(gymnet_vecenv *h, const float *d_weights, int64_t count, const float *d_x, int64_t x_stride, int64_t m,
                                       const float *d_target, float *d_grad, float *d_loss, float *d_value) {
    return guarded([&]() -> int {
    ENTER(h);
    return actor_gradient(h, false, d_weights, count, d_x, x_stride, m, nullptr, d_target, nullptr, 0.0f, 0.0f, d_grad, d_loss, d_value);
    });
}

}  // extern "C"
