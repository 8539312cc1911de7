// actor_box_compose.hpp — the Box actor's head and composition of one lane's action under a policy, as actor_box_policy.hip and
// actor_box_logd.hip both run it: one function, so the two units' actions and raw outputs are the same bits whether a log-density is
// asked for or not.  The policy is written out in actor_box_policy.hip's header and in include/gymnet_amd.h
// (gymnet_vecenv_actor_box_set_policy); policy_choose also hands out the greedy action the log-density is taken around.  Internal to
// the library.
#pragma once
#include "actor_net.hpp"

namespace gymnet {

namespace {

// the envs' own clamp (Pendulum::step): a NaN fails both compares and passes
__device__ __forceinline__ float clamp_action(float raw, float low, float high) { return raw < low ? low : (raw > high ? high : raw); }

__device__ __forceinline__ float policy_greedy(float raw, float low, float high, int32_t head) {
    if (head == GYMNET_BOX_HEAD_TANH) {                                      // wave-uniform
        const float mid = 0.5f * (low + high), half = 0.5f * (high - low);
        const float scaled = half * tanhf(raw);
        return mid + scaled;
    }
    return clamp_action(raw, low, high);
}

// compose_box_one (actor_box.hip) under a policy: words A and N are drawn only when some lane of the wave explores
__device__ __forceinline__ float policy_compose_one(float greedy, float low, float high, const BoxPolicy &pol, uint32_t explore_at_or_below, uint64_t seed,
                                                    uint64_t gl, uint64_t tick) {
    const bool explore = aux_word<true>(seed, gl, tick) <= explore_at_or_below;
    float act = greedy;
    if (__ballot(explore)) {
        const uint32_t wa = action_word<true>(seed, gl, tick);
        float drawn;
        if (pol.explore == GYMNET_BOX_EXPLORE_GAUSSIAN) {                    // wave-uniform
            const float u1 = (float)((wa >> 8) + 1u) * (1.0f / 16777216.0f);   // (0, 1]
            const float u2 = u01_24(noise_word<true>(seed, gl, tick));
            float sn, cs;
            sincos_f32<true>(6.283185307179586f * u2, sn, cs);
            const float z = sqrtf(-2.0f * logf(u1)) * cs;
            const float noise = pol.sigma * z;
            drawn = clamp_action(greedy + noise, low, high);
        } else {
            drawn = low + (high - low) * u01_24(wa);
        }
        act = explore ? drawn : greedy;
    }
    return act;
}

// history -> forward -> raw -> head -> compose, for lane i; raw receives the network's output unchanged, greedy the action after the head
template <int O>
__device__ __forceinline__ float policy_choose(const ActorNet &net, const ActorHist &hs, int32_t newest, int64_t i, float low, float high,
                                               const BoxPolicy &pol, uint32_t explore_at_or_below, uint64_t seed, uint64_t gl, uint64_t tick, float &raw,
                                               float &greedy) {
    float x[kW];
    load_input<O>(hs, newest, i, x);
    actor_forward(net, x);
    raw = x[0];
    greedy = policy_greedy(raw, low, high, pol.head);
    return policy_compose_one(greedy, low, high, pol, explore_at_or_below, seed, gl, tick);
}

// the log-density of the action a taken around the greedy action g (the five lines at the head of actor_box_logd.hip), for one lane
__device__ __forceinline__ float box_logd(float a, float g, const BoxLogd &ld) {
    const float d = (a - g) * ld.inv_sigma;
    const float h = -0.5f * d;
    return __builtin_fmaf(h, d, ld.c);
}

}  // namespace

}  // namespace gymnet
