// actor_optim.hpp — what a call to gymnet_vecenv_actor_apply_gradient is refused for, and the scalars its kernel (actor_optim.hip) takes.
// Host-only and pure as actor_grad.hpp is: no HIP type, no global, nothing read but the arguments.  This is the only place that refuses
// the call or forms a scalar of its arithmetic.
#pragma once
#include <cmath>
#include <cstdint>

namespace gymnet {

constexpr int kOptimThreads = 1024;               // the one workgroup of a call: sixteen waves
constexpr int kOptimPerThread = 8;                // thread i owns the elements i, i + 1024, ..: at most 8 of them
constexpr int64_t kOptimMaxParams = (int64_t)kOptimThreads * kOptimPerThread;      // 8192 = kGradMaxParams (asserted in actor_optim.hip)

enum OptimRule : int32_t { kOptimSgd = 0, kOptimAdadelta = 1, kOptimAdam = 2 };    // GYMNET_OPT_SGD / _ADADELTA / _ADAM

struct ActorOptimCall {                           // the call's arguments; pointers as integers, 0 = NULL
    int32_t rule;
    uintptr_t weights, grad, state, norm;
    int64_t count, step;
    float lr, p0, p1, eps, weight_decay, max_grad_norm;
};

// whether the rule reads and writes d_state at all: every rule but SGD without momentum
inline bool optim_uses_state(int32_t rule, float p0) { return rule != kOptimSgd || p0 != 0.0f; }

// NULL: the call is accepted; else why it is refused (GYMNET_ERR_INVALID_ARG).  Nothing is written by a refused call.
inline const char *actor_optim_refusal(const ActorOptimCall &c) {
    if (!c.weights || !c.grad) return "d_weights / d_grad is null";
    if (c.count < 1 || c.count > kOptimMaxParams) return "count outside [1, 8192]";
    if (c.rule != kOptimSgd && c.rule != kOptimAdadelta && c.rule != kOptimAdam) return "unknown rule";
    if (!(c.p0 >= 0.0f && c.p0 < 1.0f))           // (a NaN fails every comparison)
        return c.rule == kOptimSgd ? "momentum (p0) outside [0, 1)" : c.rule == kOptimAdadelta ? "rho (p0) outside [0, 1)" : "beta1 (p0) outside [0, 1)";
    if (c.rule == kOptimAdam && !(c.p1 >= 0.0f && c.p1 < 1.0f)) return "beta2 (p1) outside [0, 1)";
    const bool stateful = optim_uses_state(c.rule, c.p0);
    if (stateful && !c.state) return "d_state is null and the rule needs it";
    if ((c.weights | c.grad | c.state | c.norm) & 3u) return "a pointer is not 4-byte aligned";
    // [begin, end) of every buffer the kernel touches; a state the rule does not use is not touched
    const uintptr_t n = (uintptr_t)c.count * sizeof(float);
    const uintptr_t at[4] = {c.weights, c.grad, stateful ? c.state : 0, c.norm};
    const uintptr_t len[4] = {n, n, (c.rule == kOptimSgd ? 1 : 2) * n, sizeof(float)};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (at[i] && at[j] && at[i] < at[j] + len[j] && at[j] < at[i] + len[i]) return "d_weights, d_grad, d_state and d_norm must not overlap";
    if (c.rule == kOptimAdam && c.step < 1) return "step < 1";
    if (!(std::isfinite(c.lr) && c.lr >= 0.0f)) return "lr is negative or not finite";
    if (!(std::isfinite(c.eps) && c.eps >= 0.0f)) return "eps is negative or not finite";
    if (!(std::isfinite(c.weight_decay) && c.weight_decay >= 0.0f)) return "weight_decay is negative or not finite";
    if (c.rule == kOptimAdadelta && c.eps == 0.0f) return "AdaDelta needs eps > 0";
    if (!(c.max_grad_norm >= 0.0f)) return "max_grad_norm is negative or NaN";
    return nullptr;
}

// The scalars of a call, each computed in float64 from the float32 arguments and rounded once.
struct OptimScalars {
    float lr;                                     // SGD, AdaDelta: lr.  Adam: lr / (1 - beta1^step)
    float p0, q0;                                 // momentum | rho | beta1, and 1 - p0
    float p1, q1;                                 // beta2 and 1 - beta2 (Adam)
    float bias2;                                  // sqrt(1 - beta2^step) (Adam)
    float eps, weight_decay;
};
inline OptimScalars optim_scalars(const ActorOptimCall &c) {
    OptimScalars s{};
    s.p0 = c.p0; s.q0 = (float)(1.0 - (double)c.p0);
    s.p1 = c.p1; s.q1 = (float)(1.0 - (double)c.p1);
    s.eps = c.eps; s.weight_decay = c.weight_decay;
    s.lr = c.lr; s.bias2 = 1.0f;
    if (c.rule == kOptimAdam) {
        s.lr = (float)((double)c.lr / (1.0 - std::pow((double)c.p0, (double)c.step)));
        s.bias2 = (float)std::sqrt(1.0 - std::pow((double)c.p1, (double)c.step));
    }
    return s;
}

}  // namespace gymnet
