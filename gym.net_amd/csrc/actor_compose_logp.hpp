// actor_compose_logp.hpp — the Discrete actor's composition of one lane's action together with the log-probability of that action, as
// actor_logp.hip and actor_value.hip both run it: one function, so the two units' actions and logp are the same bits.  The quantity is
// written out in actor_logp.hip's header and in include/gymnet_amd.h (gymnet_vecenv_actor_act_logp_device).  Internal to the library.
#pragma once
#include "actor_net.hpp"
#include "exp_neg.hpp"
#include "log_pos.hpp"

namespace gymnet {

namespace {

// explore_compose_one (actor_softmax.hip) for one lane, which also hands out logp of the action it returns.  The scaled differences a_k
// and the running sums c_k are computed before the coin: the draw reads them where the wave draws, logp reads them always
__device__ __forceinline__ int32_t compose_one_logp(const float (&x)[kW], int32_t action_n, const ActorExplore &ex, uint32_t explore_at_or_below,
                                                    uint64_t seed, uint64_t gl, uint64_t tick, float &logp) {
    float m;
    const int32_t greedy = argmax_value(x, action_n, m);
    float a[8], c[8];
    float run = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        a[j] = 0.0f;
        if (j < action_n) {                                                  // wave-uniform
            const float d = x[j] - m;
            a[j] = d * ex.inv_tau;
            run = run + exp_neg(a[j]);
        }
        c[j] = run;
    }
    const bool explore = aux_word<true>(seed, gl, tick) <= explore_at_or_below;
    int32_t act = greedy;
    if (__ballot(explore)) {
        const uint32_t wa = action_word<true>(seed, gl, tick);
        int32_t drawn;
        if (ex.explore == GYMNET_ACTOR_EXPLORE_SOFTMAX) {                    // wave-uniform: softmax_draw's second half
            const float thr = u01_24(wa) * run;
            drawn = greedy;
#pragma unroll
            for (int j = 7; j >= 0; --j) {                                   // descending: the first k with thr < c_k wins
                if (j < action_n && thr < c[j]) drawn = j;
            }
        } else {
            drawn = (int32_t)__umulhi(wa, (uint32_t)action_n);
        }
        act = explore ? drawn : greedy;
    }
    float aj = a[0];
#pragma unroll
    for (int q = 1; q < 8; ++q) aj = q == act ? a[q] : aj;
    const float lp = aj - log_pos(run);                                      // (run < 1: not stored)
    const uint32_t bits = __builtin_bit_cast(uint32_t, lp);
    logp = __builtin_bit_cast(float, (run >= 1.0f && lp == lp) ? bits : 0x7FC00000u);
    return act;
}

}  // namespace

}  // namespace gymnet
