/* tests/cpp/actor_logp_stub.c — TEST-ONLY stand-ins for gymnet_vecenv_actor_act_logp_device and gymnet_vecenv_rollout_fused_logp_device,
 * linked beside tests/cpp/abi_stub.c (which has the rest of the C ABI) for the sanitizer build of tests/cpp/actor_logp_test.cpp.  Like
 * abi_stub.c they touch exactly what the header documents, on HOST memory: act_logp WRITES num_envs int32 actions, num_envs floats of
 * logp and, where d_logits is given, num_envs * 2 logits; the rollout WRITES steps * num_envs floats of d_rec_logp and, where given,
 * as many int32 of d_rec_actions — so a buffer the C++ side sized short is an out-of-bounds write the sanitizer sees.  A NULL logp pointer
 * writes no logp and counts as a forward to the call without it.  The stub has no actor: every handle counts as one with a Discrete actor
 * of two actions, and num_envs is what logp_stub_lanes was told.  The product never links it. */
#include <stddef.h>

#include "gymnet_amd.h"

typedef struct logp_stub_call {
    int acts, rollouts, forwarded;
    float epsilon; uint64_t seed, tick;
    int64_t steps; int32_t action_source;
} logp_stub_call;

static logp_stub_call g_last;
static int64_t g_lanes = 0;

const logp_stub_call *logp_stub_last(void) { return &g_last; }
void logp_stub_lanes(int64_t n) { g_lanes = n; }

int gymnet_vecenv_actor_act_logp_device(gymnet_vecenv *h, int32_t *d_actions, float *d_logits, float *d_logp, float epsilon, uint64_t seed,
                                        uint64_t tick) {
    if (!h || !d_actions) return GYMNET_ERR_INVALID_ARG;
    if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return GYMNET_ERR_INVALID_ARG;
    g_last.acts += 1;
    if (!d_logp) g_last.forwarded += 1;
    g_last.epsilon = epsilon; g_last.seed = seed; g_last.tick = tick;
    for (int64_t i = 0; i < g_lanes; ++i) {
        d_actions[i] = (int32_t)(i & 1);
        if (d_logits) { d_logits[2 * i] = 0.0f; d_logits[2 * i + 1] = 1.0f; }
        if (d_logp) d_logp[i] = -(float)i;
    }
    return GYMNET_OK;
}

int gymnet_vecenv_rollout_fused_logp_device(gymnet_vecenv *h, const gymnet_rollout_spec *spec, float *d_rec_logp) {
    if (!h || !spec || spec->struct_size != sizeof *spec) return GYMNET_ERR_INVALID_ARG;
    if (d_rec_logp && spec->action_source != GYMNET_ACTIONS_ACTOR) return GYMNET_ERR_INVALID_ARG;
    if (spec->steps < 0) return GYMNET_ERR_INVALID_ARG;
    g_last.rollouts += 1;
    if (!d_rec_logp) g_last.forwarded += 1;
    g_last.steps = spec->steps; g_last.action_source = spec->action_source;
    g_last.epsilon = spec->epsilon; g_last.seed = spec->action_seed; g_last.tick = spec->action_tick0;
    for (int64_t k = 0; k < spec->steps * g_lanes; ++k) {
        if (d_rec_logp) d_rec_logp[k] = -(float)k;
        if (spec->d_rec_actions) ((int32_t *)spec->d_rec_actions)[k] = (int32_t)(k & 1);
    }
    return GYMNET_OK;
}
