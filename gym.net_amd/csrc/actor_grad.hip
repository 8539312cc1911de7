// actor_grad.hip — the gradient of a minibatch loss with respect to an actor's or a critic's flat weights: the one dense contraction on
// the library's hot path, and so its one use of the matrix cores.  The contract, loss for loss, is gymnet_vecenv_actor_policy_gradient /
// gymnet_vecenv_actor_box_policy_gradient / gymnet_vecenv_actor_value_gradient / gymnet_vecenv_actor_q_gradient in include/gymnet_amd.h; what a call is refused for and
// how its launch is sized is actor_grad.hpp.
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
//   head         one thread per row, plain float32 (exp_neg.hpp, log_pos.hpp; the Box head float64, below): the row's logp / logd / value, its loss term, and dZ_L
//                unscaled into LDS, as [row][out] and transposed [out][row].  Three heads, one instantiation each (GradHead): the Discrete
//                softmax policy, the critic's squared error, and the Box actor's Gaussian policy (box_row: clamp or tanh head, the
//                log-density of actor_box_logd.hip), whose dZ_L has one live column as the critic's and which also sums g (d^2 - 1), the
//                row's share of d loss / d ln sigma, beside the loss.  The last layer of width 1 runs the plain MFMA path (one live column
//                of a 16-wide tile in forward, dW and dA): the time is in the hidden layers (docs/ledger.md §46).
//   refine       Box head only.  (a - g) / sigma^2 carries raw's error into every gradient, and a float32 raw costs more than the whole
//                of torch's float32 gradient loses.  So the hidden layers run once more in float64 on the vector unit (v_fma_f64, 4 outputs
//                a thread), from the float32 activations plus a float32 low part kept in the dZ tiles, which are free until the head; the
//                head's thread forms its row's raw, the head, the log-density and the objective in float64, and the row's loss term, sigma
//                term and dZ_L are summed in float64 over the block (db_L[0] too) and rounded once.  The backward pass stays float32 MFMA.
//                This instantiation takes 209 + 88 registers, one wave a SIMD where the others have two, and 3.7 times a float32 head's time at
//                m = 2^20 (docs/ledger.md §46): what the accuracy costs.
//   q targets    Q head only (gymnet_vecenv_actor_q_gradient), ahead of everything above: the block's own tiles of x_next forward-only under
//                the online weights (double DQN's argmax) and under the target weights (y), the weights restaged in between, each row's
//                index and target kept in d_y by the one thread that owns the row (q_targets).  Then the passes above run over x, the
//                head being Huber's of Q(x)[a] - y: one live column of dZ_L, plain float32.  162 registers, two waves a SIMD.
//   backward     last layer to first: dW_l += dZ_l^T A_l (M = outputs, N = inputs, K = the 16 rows: four instructions a tile) into
//                accumulators that stay in registers across all of the block's tiles — at most 16 tiles a layer, tile q of a layer with
//                wave q % 4 in slot q / 4; db_l as column sums by wave 0; dA_l = dZ_l W_l (M = rows, N = inputs, K = outputs) from the
//                transposed dZ, masked by A_l > 0 into dZ_{l-1}.
//   reduction    each block writes its partial gradient and loss once, to scratch [b][count + 1]; actor_grad_reduce_kernel sums the G
//                partials of a parameter in block order (in a double, rounded once), divides by m and writes d_grad / d_loss.  No
//                atomics: the same inputs give the same bits.  The Box head's sigma term goes to a [kGradBlocks] tail behind the
//                partials (their layout is the same for every head), written once per block and summed the same way by one more
//                thread of the reduce kernel, only where d_grad_log_sigma was given.
// The FP32 MFMA keeps float32 products and sums (no reduced-precision type anywhere), but sums in another order than actor_forward's fmaf
// chain: logp / value agree with the rollout's records to rounding, not bit for bit.
//
// Out of scope: action dimensions above 1, a per-lane sigma, noise before the tanh head (a squashed Gaussian), PPO value clipping, a trunk
// shared between actor and critic, gradients accumulated across calls, the optimiser step, fusing the rows= gather of
// gymnet_rollout_inputs_device into this kernel, float64 networks; and of the Q head: per-row importance weights (prioritised replay), a
// soft (Polyak) target update, dueling heads, bootstrapping through a time limit (there is no boot for Q), a Box actor.
#include "actor_grad.hpp"
#include "actor_box_compose.hpp"
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
    const float *aux;                             // policy, box: coef; value: target
    const float *logp_old;                        // policy: logp_old, box: logd_old; or null
    float clip, entropy_coef, inv_tau;
    int32_t action_n;
    float *scratch;                               // [blocks][count + 1]; box: the sigma terms [blocks] at kGradSigmaAt
    float *row_out;                               // logp / logd / value [m], or null
    const float *box_actions;                     // box: the actions taken, after the clamp
    float low, high, entropy;                     // box: the env's bounds; H = ln sigma + (1 + ln 2 pi) / 2
    int32_t box_head;
    BoxLogd ld;                                   // box: inv_sigma and c (box_logd_args)
};

// what the Q instantiation alone takes behind GradArgs (w: the online weights; x, actions, row_out = d_q as above)
struct GradQArgs : GradArgs {
    const float *w_target;                        // the target network's weights (== w: one network)
    const float *x_next;
    int64_t x_next_stride;
    const float *reward;
    const uint8_t *done;
    float gamma, delta;
    int32_t double_q;
    float *y;                                     // [m]: row i is written and read by one thread of one block only (see `target`)
};
template <int HEAD> struct GradArgsOf { typedef GradArgs type; };
template <> struct GradArgsOf<kGradQ> { typedef GradQArgs type; };

// D += A B for A [16][4], B [4][16], D [16][16]: lane (i, k) = (lane % 16, lane / 16) gives A[i][k] and B[k][i], and holds D[4 * k + r][i] in d[r]
__device__ __forceinline__ floatx4 mfma(float a, float b, floatx4 d) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, d, 0, 0, 0); }

// exp(d) for either sign from exp_neg
__device__ __forceinline__ float exp_any(float d) { return d <= 0.0f ? exp_neg(d) : 1.0f / exp_neg(-d); }

// what both policy heads make of a row's log-probability (or log-density): the row's objective s_i and g = d s_i / d logp
__device__ __forceinline__ void row_objective(const GradArgs &a, int64_t row, float logp, float &obj, float &g) {
    const float coef = a.aux[row];
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
}

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
    float obj, g;
    row_objective(a, row, logp, obj, g);
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

// one row of the Box actor's Gaussian policy loss, in float64 from the refined raw (see `refine` in the header): the row's loss term
// -(s + entropy_coef * H), its logd (the five lines of actor_box_logd.hip), d loss term / d raw, and the row's share g * (d^2 - 1) of
// d s / d ln sigma.  A NaN action or raw makes all four NaN: every factor below is a product
__device__ __forceinline__ double box_row(const GradArgs &a, int64_t row, double raw, double &logd, double &dz, double &dsigma) {
    const double low = a.low, high = a.high, inv_sigma = a.ld.inv_sigma;
    double greedy, slope;                                                    // the action after the head, d greedy / d raw
    if (a.box_head == GYMNET_BOX_HEAD_TANH) {                                // wave-uniform
        // tanh = (1 - u) / (1 + u) and 1 - tanh^2 = 4 u / (1 + u)^2 with u = exp(-2 |raw|): one exp, and no cancellation where the
        // head saturates.  A NaN raw makes u, and so everything below, NaN
        const double u = exp(-2.0 * __builtin_fabs(raw));
        greedy = 0.5 * (low + high) + 0.5 * (high - low) * __builtin_copysign((1.0 - u) / (1.0 + u), raw);
        slope = 0.5 * (high - low) * ((4.0 * u) / ((1.0 + u) * (1.0 + u)));
    } else {
        greedy = raw < low ? low : (raw > high ? high : raw);
        slope = (raw >= low ? 1.0 : 0.0) * (raw <= high ? 1.0 : 0.0);        // inclusive at both bounds
    }
    const double d = ((double)a.box_actions[row] - greedy) * inv_sigma;
    logd = __builtin_fma(-0.5 * d, d, (double)a.ld.c);
    const double coef = a.aux[row];
    double obj = coef * logd, g = coef;                                      // row_objective, in float64
    if (a.logp_old) {                                                        // wave-uniform
        const double r = exp(logd - (double)a.logp_old[row]);
        const double lo = 1.0 - (double)a.clip, hi = 1.0 + (double)a.clip;
        const double u = r * coef, c = (r < lo ? lo : (r > hi ? hi : r)) * coef;
        obj = u <= c ? u : c;                                                // ties go to the unclipped term
        g = u <= c ? u : 0.0;
    }
    if (logd != logd) { obj = logd; g = logd; }                              // (a compare with a NaN chose the clipped term)
    dz = -(g * ((d * inv_sigma) * slope));
    dsigma = g * (d * d - 1.0);
    return -(obj + (double)a.entropy_coef * (double)a.entropy);
}

// the sum over threads 0 .. 15 of a wave, in one fixed order
__device__ __forceinline__ double sum16(double v) {
#pragma unroll
    for (int s = 8; s > 0; s >>= 1) v = v + __shfl_xor(v, s, 16);
    return v;
}

// the caller's flat W_l [out][in] at `w` into LDS at their pitch, and the thread's four bias values (output 16 * wave + li of each layer).
// Only weight positions are written: the zeros between rows and behind the last matrix stay from the kernel's entry
__device__ __forceinline__ void stage_weights(const GradNet &net, const float *w, float *sW, float (&bias)[kL], int tid, int wave, int li) {
#pragma unroll
    for (int l = 0; l < kL; ++l) {
        bias[l] = 0.0f;
        if (l < net.layers) {                                                // wave-uniform
            const int32_t win = net.win[l], wout = net.wout[l];
            const float *wl = w + net.off[l];
            for (int e = tid; e < wout * win; e += 256) {
                const int o = e / win, j = e - o * win;
                sW[net.lds[l] + o * net.pitch[l] + j] = wl[e];
            }
            const int o = 16 * wave + li;
            if (o < wout) bias[l] = wl[wout * win + o];
        }
    }
    __syncthreads();
}

// A_0 = the tile of x that starts at row0, +0 beyond m and beyond win
__device__ __forceinline__ void load_tile(const GradNet &net, const float *x, int64_t x_stride, int64_t row0, int64_t m, float *sA0, int tid) {
#pragma unroll
    for (int q = 0; q < kR * kGradMaxWidth / 256; ++q) {
        const int e = tid + 256 * q, r = e >> 6, c = e & 63;
        const int64_t row = row0 + r;
        sA0[r * kP + c] = (row < m && c < net.win[0]) ? x[row * x_stride + c] : 0.0f;
    }
    __syncthreads();
}

// the forward pass over the tile in sA[0] under the weights in sW: A_{l+1} into sA[l + 1], the last layer's values into sZ
__device__ __forceinline__ void forward_tile(const GradNet &net, const float *sW, float (*sA)[kR * kP], float *sZ, const float (&bias)[kL], int wave,
                                             int li, int lk) {
#pragma unroll
    for (int l = 0; l < kL; ++l) {
        if (l < net.layers) {                                                // wave-uniform
            const int32_t win = net.win[l], wout = net.wout[l];
            const bool hidden = l + 1 < net.layers;
            if (16 * wave < wout) {                                          // wave-uniform: output tile `wave`
                const int o = 16 * wave + li;
                const bool ok = o < wout;
                const float *wrow = sW + net.lds[l] + (ok ? o : 0) * net.pitch[l] + lk;
                const float *arow = sA[l] + li * kP + lk;
                const int nch = (win + 3) >> 2;
                floatx4 z = floatx4{bias[l], bias[l], bias[l], bias[l]};
#pragma unroll
                for (int c = 0; c < kGradMaxWidth / 4; ++c) {
                    if (c < nch) {                                           // wave-uniform
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
}

// the Q head's target passes over the block's own tiles, before its gradient pass: y_i into a.y (the contract: gymnet_vecenv_actor_q_gradient).
//   select   double_q only, under the online weights: the forward over the x_next tiles; thread t < 16 of a tile takes the argmax of its
//            row of sZ and leaves the index, as an int's bits, in a.y[row]
//   target   under the target weights: the forward over the x_next tiles again; the same thread forms qn — the max, or the entry at the
//            index it left, selected by compare — and writes y over it
// Block b walks the tiles b, b + G, .. in every pass and thread t takes row t of a tile, so a.y[row] is written and read back by one thread
// only, in program order: no fence, no grid sync, no second launch, nothing sized by m.  Weights are restaged (<= 38 KB from L2) only where
// the next pass runs under another vector; `staged` names the one in LDS on return.  A done row's x_next may hold NaN: a row of the
// MFMA forward reads its own row of A only, max and argmax let no NaN win, and y is a select
__device__ __forceinline__ void q_targets(const GradQArgs &a, float *sW, float (*sA)[kR * kP], float *sZ, float (&bias)[kL], const float *&staged,
                                          int tid, int wave, int li, int lk) {
    const GradNet &net = a.net;
    const int32_t n = a.action_n;
    for (int pass = a.double_q ? 0 : 1; pass < 2; ++pass) {                  // block-uniform
        const float *w = pass == 0 ? a.w : a.w_target;
        if (w != staged) {                                                   // (every read of sW is behind a barrier: forward_tile ends on one)
            stage_weights(net, w, sW, bias, tid, wave, li);
            staged = w;
        }
        for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
            const int64_t row0 = tile * kR;
            load_tile(net, a.x_next, a.x_next_stride, row0, a.m, sA[0], tid);
            forward_tile(net, sW, sA, sZ, bias, wave, li, lk);
            // the next tile's forward writes sZ only behind load_tile's barrier, which these threads reach after their reads
            const int64_t row = row0 + tid;
            if (tid < kR && row < a.m) {
                float best = sZ[tid * kP];
                int32_t at = 0;
#pragma unroll
                for (int k = 1; k < kActorMaxActions; ++k) {
                    const float v = sZ[tid * kP + k];
                    if (k < n && v > best) { best = v; at = k; }             // strict >, from index 0: the lowest index wins a tie, a NaN never
                }
                if (pass == 0) {
                    a.y[row] = __builtin_bit_cast(float, at);
                } else {
                    float qn = best;
                    if (a.double_q) {
                        const int32_t pick = __builtin_bit_cast(int32_t, a.y[row]);
#pragma unroll
                        for (int k = 0; k < kActorMaxActions; ++k) qn = k == pick ? sZ[tid * kP + k] : qn;
                    }
                    const float r = a.reward[row];
                    a.y[row] = a.done[row] != 0 ? r : __builtin_fmaf(a.gamma, qn, r);
                }
            }
        }
    }
}

// one row of the Huber TD loss: z -> dz (one live column, or NaN in every column of an action outside the space), the row's loss term, its q
__device__ __forceinline__ float q_row(const GradQArgs &a, int64_t row, float (&z)[16], float &q) {
    const int32_t n = a.action_n;
    const int32_t act = a.actions[row];
    const bool bad = act < 0 || act >= n;                                    // never an index: selected by compare below
    const float nan = __builtin_bit_cast(float, 0x7FC00000u);
    float qa = 0.0f;
#pragma unroll
    for (int k = 0; k < kActorMaxActions; ++k) qa = k == act ? z[k] : qa;
    q = bad ? nan : qa;
    const float td = q - a.y[row];
    const float mag = __builtin_fabsf(td);
    // a NaN td fails the compare and stays NaN in the linear branch; delta = +inf takes the square for every finite td
    const float term = mag <= a.delta ? 0.5f * (td * td) : a.delta * (mag - 0.5f * a.delta);
    const float g = td > a.delta ? a.delta : (td < -a.delta ? -a.delta : td);                  // a NaN td passes both compares
#pragma unroll
    for (int k = 0; k < 16; ++k) z[k] = (k < kActorMaxActions && k < n) ? (bad ? nan : (k == act ? g : 0.0f)) : 0.0f;
    return term;
}

template <int HEAD>                                                         // a GradHead (an int: the listing names the instantiations <0>, <1>, <2>, <3>)
__global__ __launch_bounds__(256) void actor_grad_kernel(const typename GradArgsOf<HEAD>::type a) {
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
    if constexpr (HEAD == kGradQ) {
        // the target passes first (q_targets), then the online weights for the gradient pass, restaged unless they are the ones in LDS
        const float *staged = nullptr;
        q_targets(a, sW, sA, sZ, bias, staged, tid, wave, li, lk);
        if (staged != a.w) stage_weights(net, a.w, sW, bias, tid, wave, li);
    } else {
        stage_weights(net, a.w, sW, bias, tid, wave, li);
    }

    floatx4 acc[kL][4];                                                      // dW_l tile q = wave + 4 * slot, across all of the block's tiles
#pragma unroll
    for (int l = 0; l < kL; ++l)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[l][s] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
    float db[kL] = {0.0f, 0.0f, 0.0f, 0.0f};                                 // wave 0: db_l[tid]
    float loss = 0.0f;                                                       // threads 0 .. 15: the loss terms of row tid of every tile
    double loss_d = 0.0, sigma_d = 0.0, db_d = 0.0;                          // box, threads 0 .. 15: its loss terms, g * (d^2 - 1) and dZ_L

    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t row0 = tile * kR;
        // ---- A_0 = the tile of x, then the forward pass
        load_tile(net, a.x, a.x_stride, row0, a.m, sA[0], tid);
        forward_tile(net, sW, sA, sZ, bias, wave, li, lk);
        // ---- box, refine: the hidden layers once more in float64 on the vector unit.  A_{l+1} = hi + lo, hi the float32 value the MFMA
        // pass left in sA, lo = relu(float64 row) - hi in the dZ tiles, free until the head: lo_{l+1} in sZT for even l, in sZ for odd.
        // Thread (row li, outputs lk + 4 * wave + 16 * q): activations along a row, four weight rows a wave, no bank conflicts
        if constexpr (HEAD == kGradBox) {
#pragma unroll
            for (int l = 0; l < kL - 1; ++l) {
                if (l + 1 < net.layers) {                                    // wave-uniform
                    const int32_t win = net.win[l], wout = net.wout[l];
                    const float *wl = a.w + net.off[l];
                    const float *lo_in = (l & 1) ? sZT : sZ;
                    float *lo_out = (l & 1) ? sZ : sZT;
                    double z[4];
                    const float *wrow[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int o = lk + 4 * wave + 16 * q;
                        z[q] = o < wout ? (double)wl[wout * win + o] : 0.0;
                        wrow[q] = sW + net.lds[l] + (o < wout ? o : 0) * net.pitch[l];
                    }
#pragma unroll 2
                    for (int j = 0; j < win; ++j) {
                        double av = (double)sA[l][li * kP + j];
                        if (l > 0) av = av + (double)lo_in[li * kP + j];
#pragma unroll
                        for (int q = 0; q < 4; ++q) z[q] = __builtin_fma(av, (double)wrow[q][j], z[q]);
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int o = lk + 4 * wave + 16 * q;
                        if (o < wout) lo_out[li * kP + o] = (float)((z[q] > 0.0 ? z[q] : 0.0) - (double)sA[l + 1][li * kP + o]);
                    }
                    __syncthreads();
                }
            }
        }
        // ---- head: one thread per row
        if (tid < kR) {
            const int64_t row = row0 + tid;
            float z[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) z[k] = 0.0f;
            if (row < a.m) {
                if constexpr (HEAD == kGradPolicy) {
#pragma unroll
                    for (int k = 0; k < kActorMaxActions; ++k) z[k] = sZ[tid * kP + k];
                    float logp;
                    loss = loss + policy_row(a, row, z, logp);
                    if (a.row_out) a.row_out[row] = logp;
                } else if constexpr (HEAD == kGradQ) {
#pragma unroll
                    for (int k = 0; k < kActorMaxActions; ++k) z[k] = sZ[tid * kP + k];
                    float q;
                    loss = loss + q_row(a, row, z, q);
                    if (a.row_out) a.row_out[row] = q;
                } else if constexpr (HEAD == kGradBox) {
                    // raw = A_L W_L[0] + b_L[0] in float64 from hi + lo; the other threads' lo rows are read before any dZ is written
                    // below (one wave, in program order)
                    const int L = net.layers - 1;
                    const int32_t win = net.win[L];
                    const float *lo_in = (L & 1) ? sZT : sZ;
                    double raw = (double)a.w[net.off[L] + net.wout[L] * win];
#pragma unroll 2
                    for (int j = 0; j < win; ++j) {
                        double av = (double)sA[L][tid * kP + j];
                        if (L > 0) av = av + (double)lo_in[tid * kP + j];
                        raw = __builtin_fma(av, (double)sW[net.lds[L] + j], raw);
                    }
                    double logd, dz, ds;
                    loss_d = loss_d + box_row(a, row, raw, logd, dz, ds);
                    sigma_d = sigma_d + ds;
                    db_d = db_d + dz;
                    z[0] = (float)dz;
                    if (a.row_out) a.row_out[row] = (float)logd;
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
    if constexpr (HEAD == kGradBox) {
        // the block's loss, sigma term and db_L[0] from the rows' float64 terms, each rounded once; thread 0 wrote db_L[0] from the
        // float32 column sums above and replaces it here
        if (tid < kR) {
            const double ls = sum16(loss_d), ss = sum16(sigma_d), bs = sum16(db_d);
            if (tid == 0) {
                const int L = net.layers - 1;
                part[net.count] = (float)ls;
                part[net.off[L] + net.wout[L] * net.win[L]] = (float)bs;
                a.scratch[kGradSigmaAt + blockIdx.x] = (float)ss;
            }
        }
    } else {
        if (tid < kR) sLoss[tid] = loss;
        __syncthreads();
        if (tid == 0) {
            float sum = 0.0f;
#pragma unroll
            for (int r = 0; r < kR; ++r) sum = sum + sLoss[r];
            part[net.count] = sum;
        }
    }
}

// parameter i (i == count: the loss): the blocks' partials in block order, over m.  The running sum is a double, rounded to float32 once at the
// end: up to 512 partials of either sign summed in float32 lose several units in the last place, more than torch's own float32 gradient.
// i == count + 1, where the Box call asked for it (the grid is one thread longer then): the blocks' sigma terms behind the partials, in the
// same way, as d loss / d ln sigma = -mean(g (d^2 - 1)) - entropy_coef
__global__ __launch_bounds__(256) void actor_grad_reduce_kernel(const float *__restrict__ scratch, int32_t blocks, int32_t count, double m,
                                                                float *__restrict__ grad, float *__restrict__ loss,
                                                                float *__restrict__ grad_log_sigma, float entropy_coef) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > count) {
        if (i == count + 1 && grad_log_sigma) {
            double sum = 0.0;
            for (int b = 0; b < blocks; ++b) sum = sum + (double)scratch[kGradSigmaAt + b];
            *grad_log_sigma = (float)(-(sum / m) - (double)entropy_coef);
        }
        return;
    }
    double sum = 0.0;
    for (int b = 0; b < blocks; ++b) sum = sum + (double)scratch[(int64_t)b * (count + 1) + i];
    const float out = (float)(sum / m);
    if (i < count) grad[i] = out;
    else if (loss) *loss = out;
}

// the handle's scratch (actor_grad.hpp kGradScratchFloats), allocated on the first call and gone with the actor
int grad_scratch(gymnet_vecenv *h, float *&scratch) {
    Actor &ac = *h->actor;
    if (!ac.grad_scratch) {
        ac.grad_scratch = static_cast<float *>(ac.mem.take(sizeof(float) * (size_t)kGradScratchFloats));
        if (!ac.grad_scratch) return fail(h, GYMNET_ERR_OOM, "hipMalloc of the gradient scratch failed");
    }
    scratch = ac.grad_scratch;
    return GYMNET_OK;
}

constexpr const char *kGradCallName[] = {"actor_value_gradient", "actor_policy_gradient", "actor_box_policy_gradient", "actor_q_gradient"};

// d_actions: int32 for the Discrete call, float32 for the Box call; d_grad_log_sigma: the Box call's, or null
int actor_gradient(gymnet_vecenv *h, GradHead head, const float *d_weights, int64_t count, const float *d_x, int64_t x_stride, int64_t m,
                   const void *d_actions, const float *d_aux, const float *d_logp_old, float clip, float entropy_coef, float *d_grad, float *d_loss,
                   float *d_row_out, float *d_grad_log_sigma) {
    const Actor *ac = h->actor;
    const bool policy = head != kGradValue;
    const ActorNet *an = !ac ? nullptr : (policy ? &ac->net : &ac->critic);
    const bool has_net = an && an->layers > 0;
    const ActorGradCall c{head, ac != nullptr, ac && ac->box, ac && ac->has_critic(), ac ? ac->sigma : 0.0f, !ac ? 0 : (policy ? ac->count : ac->critic_count),
                          has_net ? an->win[0] : 0, count, x_stride, m, (uintptr_t)d_weights, (uintptr_t)d_x, (uintptr_t)d_actions, (uintptr_t)d_aux,
                          (uintptr_t)d_logp_old, (uintptr_t)d_grad, clip, entropy_coef};
    if (const char *why = actor_grad_refusal(c)) return fail(h, GYMNET_ERR_INVALID_ARG, "%s: %s", kGradCallName[head], why);
    GradArgs a{};
    if (grad_net_shape(a.net, an->layers, an->win, an->wout) > kGradLdsWeights || a.net.count != count)
        return fail(h, GYMNET_ERR_HIP, "actor gradient: the network does not fit the kernel's LDS plan");
    const ActorGradForm f = pick_actor_grad_form(m);
    ST_TRY(grad_scratch(h, a.scratch));
    a.w = d_weights; a.x = d_x; a.x_stride = x_stride; a.m = m; a.tiles = f.tiles;
    a.aux = d_aux; a.logp_old = d_logp_old;
    a.clip = clip; a.entropy_coef = entropy_coef; a.inv_tau = ac->inv_tau; a.action_n = an->action_n;
    a.row_out = d_row_out;
    if (head == kGradBox) {
        a.box_actions = static_cast<const float *>(d_actions);
        a.low = h->desc->action_low; a.high = h->desc->action_high; a.box_head = ac->head;
        a.ld = box_logd_args(ac->sigma);
        a.entropy = (float)(std::log((double)ac->sigma) + 1.41893853320467274178);      // ln sigma + (1 + ln 2 pi) / 2
        hipLaunchKernelGGL(actor_grad_kernel<kGradBox>, dim3((unsigned)f.blocks), dim3(256), 0, h->stream, a);
    } else {
        a.actions = static_cast<const int32_t *>(d_actions);
        if (policy) hipLaunchKernelGGL(actor_grad_kernel<kGradPolicy>, dim3((unsigned)f.blocks), dim3(256), 0, h->stream, a);
        else hipLaunchKernelGGL(actor_grad_kernel<kGradValue>, dim3((unsigned)f.blocks), dim3(256), 0, h->stream, a);
    }
    HIP_TRY(h, hipGetLastError());
    const int64_t outputs = count + 1 + (d_grad_log_sigma ? 1 : 0);
    hipLaunchKernelGGL(actor_grad_reduce_kernel, dim3((unsigned)((outputs + 255) / 256)), dim3(256), 0, h->stream, a.scratch, f.blocks, (int32_t)count,
                       (double)m, d_grad, d_loss, d_grad_log_sigma, entropy_coef);
    HIP_TRY(h, hipGetLastError());
    return GYMNET_OK;
}

// the Q-learning call: the same launch form, partials and reduce kernel as the calls above; the stored temperature is not read
int actor_q_gradient(gymnet_vecenv *h, const float *d_weights, const float *d_target_weights, int64_t count, const float *d_x, int64_t x_stride,
                     const float *d_x_next, int64_t x_next_stride, int64_t m, const int32_t *d_actions, const float *d_reward, const uint8_t *d_done,
                     float gamma, float huber_delta, int32_t double_q, float *d_y, float *d_grad, float *d_loss, float *d_q) {
    const Actor *ac = h->actor;
    const bool has_net = ac && ac->net.layers > 0;
    const ActorQGradCall c{ac != nullptr, ac && ac->box, ac ? ac->count : 0, has_net ? ac->net.win[0] : 0, count, x_stride, x_next_stride, m,
                           (uintptr_t)d_weights, (uintptr_t)d_x, (uintptr_t)d_x_next, (uintptr_t)d_actions, (uintptr_t)d_reward, (uintptr_t)d_done,
                           (uintptr_t)d_y, (uintptr_t)d_grad, gamma, huber_delta};
    if (const char *why = actor_q_grad_refusal(c)) return fail(h, GYMNET_ERR_INVALID_ARG, "%s: %s", kGradCallName[kGradQ], why);
    GradQArgs a{};
    if (grad_net_shape(a.net, ac->net.layers, ac->net.win, ac->net.wout) > kGradLdsWeights || a.net.count != count)
        return fail(h, GYMNET_ERR_HIP, "actor gradient: the network does not fit the kernel's LDS plan");
    const ActorGradForm f = pick_actor_grad_form(m);
    ST_TRY(grad_scratch(h, a.scratch));
    a.w = d_weights; a.x = d_x; a.x_stride = x_stride; a.m = m; a.tiles = f.tiles;
    a.actions = d_actions; a.action_n = ac->net.action_n; a.row_out = d_q;
    a.w_target = d_target_weights ? d_target_weights : d_weights;
    a.x_next = d_x_next; a.x_next_stride = x_next_stride; a.reward = d_reward; a.done = d_done;
    a.gamma = gamma; a.delta = huber_delta; a.double_q = double_q != 0; a.y = d_y;
    hipLaunchKernelGGL(actor_grad_kernel<kGradQ>, dim3((unsigned)f.blocks), dim3(256), 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(actor_grad_reduce_kernel, dim3((unsigned)((count + 1 + 255) / 256)), dim3(256), 0, h->stream, a.scratch, f.blocks, (int32_t)count,
                       (double)m, d_grad, d_loss, (float *)nullptr, 0.0f);
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
    return actor_gradient(h, kGradPolicy, d_weights, count, d_x, x_stride, m, d_actions, d_coef, d_logp_old, clip, entropy_coef, d_grad, d_loss, d_logp, nullptr);
    });
}

int gymnet_vecenv_actor_value_gradient(gymnet_vecenv *h, const float *d_weights, int64_t count, const float *d_x, int64_t x_stride, int64_t m,
                                       const float *d_target, float *d_grad, float *d_loss, float *d_value) {
    return guarded([&]() -> int {
    ENTER(h);
    return actor_gradient(h, kGradValue, d_weights, count, d_x, x_stride, m, nullptr, d_target, nullptr, 0.0f, 0.0f, d_grad, d_loss, d_value, nullptr);
    });
}

int gymnet_vecenv_actor_box_policy_gradient(gymnet_vecenv *h, const float *d_weights, int64_t count, const float *d_x, int64_t x_stride, int64_t m,
                                            const float *d_actions, const float *d_coef, const float *d_logd_old, float clip, float entropy_coef,
                                            float *d_grad, float *d_loss, float *d_logd, float *d_grad_log_sigma) {
    return guarded([&]() -> int {
    ENTER(h);
    return actor_gradient(h, kGradBox, d_weights, count, d_x, x_stride, m, d_actions, d_coef, d_logd_old, clip, entropy_coef, d_grad, d_loss, d_logd,
                          d_grad_log_sigma);
    });
}

int gymnet_vecenv_actor_q_gradient(gymnet_vecenv *h, const float *d_weights, const float *d_target_weights, int64_t count, const float *d_x,
                                   int64_t x_stride, const float *d_x_next, int64_t x_next_stride, int64_t m, const int32_t *d_actions,
                                   const float *d_reward, const uint8_t *d_done, float gamma, float huber_delta, int32_t double_q, float *d_y,
                                   float *d_grad, float *d_loss, float *d_q) {
    return guarded([&]() -> int {
    ENTER(h);
    return actor_q_gradient(h, d_weights, d_target_weights, count, d_x, x_stride, d_x_next, x_next_stride, m, d_actions, d_reward, d_done, gamma,
                            huber_delta, double_q, d_y, d_grad, d_loss, d_q);
    });
}

}  // extern "C"
