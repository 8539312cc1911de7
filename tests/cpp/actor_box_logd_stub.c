/* tests/cpp/actor_box_logd_stub.c — TEST-ONLY stand-ins for the Box actor's two log-density calls
 * (gymnet_vecenv_actor_box_act_logd_device, gymnet_vecenv_rollout_fused_box_logd_device), linked beside tests/cpp/abi_stub.c (which has
 * the rest of the C ABI) for the sanitizer build of tests/cpp/actor_box_logd_test.cpp.  Like abi_stub.c they touch exactly what the
 * header documents, on HOST memory: act WRITES num_envs floats of actions and, where given, num_envs floats of raw and of logd; the
 * rollout steps * num_envs floats of each record pointer given and of d_rec_actions — so a buffer sized short is an out-of-bounds write
 * the sanitizer sees.  A NULL d_logd, or both record pointers NULL, counts as a forward to the call without them.  The stub has no actor:
 * every handle counts as one with a Box actor, with a critic after logd_stub_setup(n, 1).  The product never links it. */
#include <stddef.h>

#include "gymnet_amd.h"

typedef struct logd_stub_call {
    int calls, forwarded;
    float epsilon; uint64_t seed, tick;
    int64_t steps; int32_t action_source;
    const float *logd_at, *value_at;
} logd_stub_call;

static logd_stub_call g_last;
static int64_t g_lanes = 0;
static int g_critic = 0;

const logd_stub_call *logd_stub_last(void) { return &g_last; }
void logd_stub_setup(int64_t n, int critic) { g_lanes = n; g_critic = critic; }

int gymnet_vecenv_actor_box_act_logd_device(gymnet_vecenv *h, float *d_actions, float *d_raw, float *d_logd, float epsilon, uint64_t seed,
                                            uint64_t tick) {
    if (!h || !d_actions) return GYMNET_ERR_INVALID_ARG;
    if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return GYMNET_ERR_INVALID_ARG;
    g_last.calls += 1;
    if (!d_logd) g_last.forwarded += 1;
    g_last.epsilon = epsilon; g_last.seed = seed; g_last.tick = tick; g_last.logd_at = d_logd;
    for (int64_t i = 0; i < g_lanes; ++i) {
        d_actions[i] = 0.5f * (float)i;
        if (d_raw) d_raw[i] = 100.0f + (float)i;
        if (d_logd) d_logd[i] = -(float)i;
    }
    return GYMNET_OK;
}

int gymnet_vecenv_rollout_fused_box_logd_device(gymnet_vecenv *h, const gymnet_rollout_spec *spec, float *d_rec_logd, float *d_rec_value) {
    if (!h || !spec || spec->struct_size != sizeof *spec) return GYMNET_ERR_INVALID_ARG;
    if ((d_rec_logd || d_rec_value) && spec->action_source != GYMNET_ACTIONS_ACTOR) return GYMNET_ERR_INVALID_ARG;
    if (d_rec_value && !g_critic) return GYMNET_ERR_INVALID_ARG;
    if (spec->steps < 0) return GYMNET_ERR_INVALID_ARG;
    g_last.calls += 1;
    if (!d_rec_logd && !d_rec_value) g_last.forwarded += 1;
    g_last.steps = spec->steps; g_last.action_source = spec->action_source;
    g_last.epsilon = spec->epsilon; g_last.seed = spec->action_seed; g_last.tick = spec->action_tick0;
    g_last.logd_at = d_rec_logd; g_last.value_at = d_rec_value;
    for (int64_t k = 0; k < spec->steps * g_lanes; ++k) {
        if (d_rec_logd) d_rec_logd[k] = -(float)k;
        if (d_rec_value) d_rec_value[k] = (float)k;
        if (spec->d_rec_actions) ((float *)spec->d_rec_actions)[k] = 0.5f * (float)k;
    }
    return GYMNET_OK;
}
