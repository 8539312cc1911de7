// actor_grad.hpp — what a call to gymnet_vecenv_actor_policy_gradient / gymnet_vecenv_actor_box_policy_gradient /
// gymnet_vecenv_actor_value_gradient / gymnet_vecenv_actor_q_gradient is refused for, how its rows are dealt to the workgroups of actor_grad.hip, and where that kernel
// keeps a network in LDS.  Host-only and pure as rollout_inputs.hpp is: no HIP type, no global, nothing read but the arguments
// (rollout_plan.hpp, as pure, for the sigmas a log-density is defined for).  This is the only place that refuses a call or sizes its launch.
#pragma once
#include <cmath>
#include <cstdint>

#include "rollout_plan.hpp"

namespace gymnet {

constexpr int kGradRows = 16;                     // R: rows of x per tile, the M (forward) and K (dW) of the 16x16x4 MFMA
constexpr int kGradBlocks = 512;                  // the most workgroups a call launches: two for each of an MI355X's 256 CUs (with one,
                                                  // m = 2^20 takes 1.7 times as long: docs/ledger.md §45).  A constant, never read from the
                                                  // device: the summation order, and so every bit, follows from m alone
constexpr int kGradMaxLayers = 4, kGradMaxWidth = 64, kGradMaxParams = 8192;      // (actor_net.hpp's limits)

// LDS pitch of a row of `w` floats: the least multiple of 4 that is >= w and whose quarter is odd (4, 12, 20, .. 68).  Every MFMA operand is
// read in one of two patterns by the lanes (i, k) = (lane % 16, lane / 16) of a wave:
//   along a row:    row i,          column c + k        address i * p + k         forward: activations and weights
//   down a column:  row c + 4 * k,  column i            address 4 * k * p + i     dW: dZ and activations; dA: dZ^T and weights
// With p = 4 * odd, i * p runs through all sixteen multiples of 4 modulo 64 and 4 * p is 16 or 48 modulo 64, so in both patterns the 64
// lanes of a ds_read_b32 fall into 64 different banks of the CU's 64 x 4-byte LDS banks.  (Served as two halves over 32 banks, the first
// pattern would be a two-way conflict and the second none.)  The K order of the second pattern — rows c, c + 4, c + 8, c + 12 — is free
// to choose: both operands of an instruction use the same one, and a sum does not care.
inline constexpr int grad_pitch(int w) { return 4 * ((((w + 3) >> 2) & 1) ? ((w + 3) >> 2) : ((w + 3) >> 2) + 1); }

constexpr int kGradPitch = grad_pitch(kGradMaxWidth);        // 68: an activation row
constexpr int kGradPitchT = grad_pitch(kGradRows);           // 20: a row of dZ^T
// floats of LDS for the weight matrices at their pitches (biases live in registers): the largest over every network of at most 4 layers,
// widths <= 64 and <= 8192 parameters is 9460, at widths 5-61-45-45-64 (searched exhaustively); a call whose network needed more would be
// refused as an internal error
constexpr int kGradLdsWeights = 9472;
// static LDS of the main kernel in bytes: weights, four activation tiles, dZ, dZ^T, sixteen loss terms = 64 832 <= 65 536
constexpr int kGradLdsBytes = 4 * (kGradLdsWeights + kGradMaxLayers * kGradRows * kGradPitch + kGradRows * kGradPitch + kGradMaxWidth * kGradPitchT + kGradRows);
static_assert(kGradLdsBytes <= 64 * 1024, "two workgroups share a CU");

// the scratch of a handle in floats: kGradBlocks partials [count + 1] of the largest network, then — behind them, so that the partial
// layout is the same for every head — one float per block for the Box head's sigma term
constexpr int64_t kGradSigmaAt = (int64_t)kGradBlocks * (kGradMaxParams + 1);
constexpr int64_t kGradScratchFloats = kGradSigmaAt + kGradBlocks;

// the loss a call differentiates, and so the head the main kernel is instantiated for
enum GradHead : int { kGradValue = 0, kGradPolicy = 1, kGradBox = 2, kGradQ = 3 };        // _value_gradient, _policy_gradient, _box_policy_gradient, _q_gradient

struct ActorGradCall {                            // the call's arguments and what it reads of the handle; pointers as integers, 0 = NULL
    GradHead head;
    bool has_actor, box, has_critic;
    float sigma;                                  // a Box actor's stored sigma (read by the Box call only)
    int64_t configured_count;                     // the parameters of the network the call differentiates
    int32_t win0;                                 // its input width
    int64_t count, x_stride, m;
    uintptr_t weights, x, actions, aux, logp_old, grad;      // aux: d_coef / d_target; logp_old: d_logp_old / d_logd_old
    float clip, entropy_coef;
};

// NULL: the call is accepted; else why it is refused (GYMNET_ERR_INVALID_ARG).  Nothing is written by a refused call.
inline const char *actor_grad_refusal(const ActorGradCall &c) {
    const bool policy = c.head != kGradValue;     // either policy call
    if (!c.has_actor) return "no actor configured";
    if (c.head == kGradPolicy && c.box) return "the policy gradient serves a Discrete actor; this handle's actor chooses Box actions";
    if (c.head == kGradBox && !c.box) return "the Box policy gradient serves a Box actor; this handle's actor chooses Discrete actions";
    if (c.head == kGradBox && !box_sigma_ok(c.sigma))
        return "the log-density needs a policy with sigma > 0 and a finite 1 / sigma (gymnet_vecenv_actor_box_set_policy)";
    if (!policy && !c.has_critic) return "no critic configured (gymnet_vecenv_actor_critic_config)";
    if (c.count != c.configured_count) return policy ? "count != the actor's parameters" : "count != the critic's parameters";
    if (c.m < 1) return "m < 1";
    if (c.x_stride < c.win0) return "x_stride < widths[0]";
    if (!c.weights || !c.x || !c.aux || !c.grad || (policy && !c.actions))
        return policy ? "d_weights / d_x / d_actions / d_coef / d_grad is null" : "d_weights / d_x / d_target / d_grad is null";
    if (policy && c.logp_old && !(c.clip >= 0.0f && c.clip < 1.0f))
        return c.head == kGradBox ? "clip must be in [0, 1) with d_logd_old" : "clip must be in [0, 1) with d_logp_old";
    if (policy && !std::isfinite(c.entropy_coef)) return "entropy_coef is not finite";
    if (c.m > INT64_MAX / 4 / c.x_stride) return "m x x_stride overflows";
    return nullptr;
}

// the Q-learning call (gymnet_vecenv_actor_q_gradient): its arguments and what it reads of the handle, as ActorGradCall
struct ActorQGradCall {
    bool has_actor, box;
    int64_t configured_count;                     // the parameters of the Discrete actor's network
    int32_t win0;                                 // its input width
    int64_t count, x_stride, x_next_stride, m;
    uintptr_t weights, x, x_next, actions, reward, done, y, grad;            // (d_target_weights, d_loss and d_q may be NULL)
    float gamma, huber_delta;
};

// NULL: the call is accepted; else why it is refused (GYMNET_ERR_INVALID_ARG).  Nothing is written by a refused call.
inline const char *actor_q_grad_refusal(const ActorQGradCall &c) {
    if (!c.has_actor) return "no actor configured";
    if (c.box) return "the Q gradient serves a Discrete actor; this handle's actor chooses Box actions";
    if (c.count != c.configured_count) return "count != the actor's parameters";
    if (c.m < 1) return "m < 1";
    if (c.x_stride < c.win0) return "x_stride < widths[0]";
    if (c.x_next_stride < c.win0) return "x_next_stride < widths[0]";
    if (!c.weights || !c.x || !c.x_next || !c.actions || !c.reward || !c.done || !c.y || !c.grad)
        return "d_weights / d_x / d_x_next / d_actions / d_reward / d_done / d_y / d_grad is null";
    if (!(c.gamma >= 0.0f && c.gamma <= 1.0f)) return "gamma must be in [0, 1]";
    if (!(c.huber_delta > 0.0f)) return "huber_delta must be > 0 (+inf: the squared error)";
    if (c.m > INT64_MAX / 4 / c.x_stride) return "m x x_stride overflows";
    if (c.m > INT64_MAX / 4 / c.x_next_stride) return "m x x_next_stride overflows";
    return nullptr;
}

struct ActorGradForm {
    int64_t tiles;                                // ceil(m / R)
    int32_t blocks;                               // G = min(tiles, kGradBlocks): block b takes tiles b, b + G, b + 2G, ..
};
inline ActorGradForm pick_actor_grad_form(int64_t m) {
    ActorGradForm f{};
    f.tiles = (m + kGradRows - 1) / kGradRows;
    f.blocks = (int32_t)(f.tiles < kGradBlocks ? f.tiles : kGradBlocks);
    return f;
}

// the network as the kernels see it: flat offsets in the caller's layout (W_l at off[l], its bias behind it) and LDS offsets at the pitch
struct GradNet {
    int32_t layers, count;
    int32_t win[kGradMaxLayers], wout[kGradMaxLayers], off[kGradMaxLayers], lds[kGradMaxLayers], pitch[kGradMaxLayers];
};
// returns the floats of LDS the weight matrices take
inline int64_t grad_net_shape(GradNet &g, int32_t layers, const int32_t *win, const int32_t *wout) {
    g = GradNet{};
    g.layers = layers;
    int64_t flat = 0, lds = 0;
    for (int l = 0; l < layers; ++l) {
        g.win[l] = win[l]; g.wout[l] = wout[l];
        g.off[l] = (int32_t)flat; g.lds[l] = (int32_t)lds; g.pitch[l] = grad_pitch(win[l]);
        flat += (int64_t)wout[l] * win[l] + wout[l];
        lds += (int64_t)wout[l] * g.pitch[l];
    }
    g.count = (int32_t)flat;
    return lds;
}

}  // namespace gymnet
