/* tests/cpp/actor_value_stub.c — TEST-ONLY stand-ins for the critic's five calls (gymnet_vecenv_actor_critic_config,
 * _actor_critic_load_device, _actor_value_device, _actor_act_value_device, gymnet_vecenv_rollout_fused_value_device), linked beside
 * tests/cpp/abi_stub.c (which has the rest of the C ABI) for the sanitizer build of tests/cpp/actor_value_test.cpp, and built alone as a
 * shared library that tests/test_actor_value_host.py hands to the Python wrapper in the library's place.  Like abi_stub.c they touch
 * exactly what the header documents, on HOST memory: value WRITES num_envs floats; act_value num_envs int32 actions and, where given,
 * num_envs floats of logp, num_envs floats of value and num_envs * 2 logits; the rollout steps * num_envs floats of d_rec_value and, where
 * given, as many of d_rec_logp and int32 of d_rec_actions — so a buffer sized short is an out-of-bounds write the sanitizer sees.  The
 * stub READS count weights and num_layers + 1 widths.  A NULL value pointer counts as a forward to the call without it and writes nothing
 * but what that call writes.  The stub has no actor: every handle counts as one with a Discrete actor of two actions whose input is
 * value_stub_lanes' `input` wide; a critic exists between a config with layers and one without.  Every call is appended to a log of call
 * ids, which is how the tests see their order.  The product never links it. */
#include <stddef.h>

#include "gymnet_amd.h"

enum { VALUE_STUB_CONFIG = 1, VALUE_STUB_LOAD = 2, VALUE_STUB_VALUE = 3, VALUE_STUB_ACT = 4, VALUE_STUB_ROLLOUT = 5 };

typedef struct value_stub_call {
    int calls, forwarded;
    int log[16];                               /* the ids of the first 16 calls, in order */
    int32_t num_layers; int64_t count; float weight_sum;
    float epsilon; uint64_t seed, tick;
    int64_t steps; int32_t action_source;
    const float *value_at;                     /* where the last value call wrote */
    int has_critic;
} value_stub_call;

static value_stub_call g_last;
static int64_t g_lanes = 0;
static int32_t g_input = 0;

const value_stub_call *value_stub_last(void) { return &g_last; }
void value_stub_lanes(int64_t n, int32_t input) { g_lanes = n; g_input = input; }
void value_stub_clear(void) { value_stub_call zero = {0}; g_last = zero; }

static void logged(int id) {
    if (g_last.calls < 16) g_last.log[g_last.calls] = id;
    g_last.calls += 1;
}

int gymnet_vecenv_actor_critic_config(gymnet_vecenv *h, int32_t num_layers, const int32_t *widths, const float *weights, int64_t count) {
    if (!h) return GYMNET_ERR_INVALID_ARG;
    if (num_layers == 0) { logged(VALUE_STUB_CONFIG); g_last.num_layers = 0; g_last.has_critic = 0; return GYMNET_OK; }
    if (num_layers < 1 || num_layers > 4 || !widths || !weights) return GYMNET_ERR_INVALID_ARG;
    if (widths[0] != g_input || widths[num_layers] != 1) return GYMNET_ERR_INVALID_ARG;
    int64_t params = 0;
    for (int l = 0; l < num_layers; ++l) params += (int64_t)widths[l + 1] * widths[l] + widths[l + 1];
    if (count != params) return GYMNET_ERR_INVALID_ARG;
    logged(VALUE_STUB_CONFIG);
    g_last.num_layers = num_layers; g_last.count = count; g_last.has_critic = 1;
    g_last.weight_sum = 0.0f;
    for (int64_t k = 0; k < count; ++k) g_last.weight_sum += weights[k];
    return GYMNET_OK;
}

int gymnet_vecenv_actor_critic_load_device(gymnet_vecenv *h, const float *d_weights, int64_t count) {
    if (!h || !d_weights || !g_last.has_critic || count != g_last.count) return GYMNET_ERR_INVALID_ARG;
    logged(VALUE_STUB_LOAD);
    g_last.weight_sum = 0.0f;
    for (int64_t k = 0; k < count; ++k) g_last.weight_sum += d_weights[k];
    return GYMNET_OK;
}

int gymnet_vecenv_actor_value_device(gymnet_vecenv *h, float *d_value) {
    if (!h || !d_value || !g_last.has_critic) return GYMNET_ERR_INVALID_ARG;
    logged(VALUE_STUB_VALUE);
    g_last.value_at = d_value;
    for (int64_t i = 0; i < g_lanes; ++i) d_value[i] = 1000.0f + (float)i;
    return GYMNET_OK;
}

int gymnet_vecenv_actor_act_value_device(gymnet_vecenv *h, int32_t *d_actions, float *d_logits, float *d_logp, float *d_value, float epsilon,
                                         uint64_t seed, uint64_t tick) {
    if (!h || !d_actions) return GYMNET_ERR_INVALID_ARG;
    if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return GYMNET_ERR_INVALID_ARG;
    if (d_value && !g_last.has_critic) return GYMNET_ERR_INVALID_ARG;
    logged(VALUE_STUB_ACT);
    if (!d_value) g_last.forwarded += 1;
    g_last.epsilon = epsilon; g_last.seed = seed; g_last.tick = tick;
    for (int64_t i = 0; i < g_lanes; ++i) {
        d_actions[i] = (int32_t)(i & 1);
        if (d_logits) { d_logits[2 * i] = 0.0f; d_logits[2 * i + 1] = 1.0f; }
        if (d_logp) d_logp[i] = -(float)i;
        if (d_value) d_value[i] = 1000.0f + (float)i;
    }
    return GYMNET_OK;
}

int gymnet_vecenv_rollout_fused_value_device(gymnet_vecenv *h, const gymnet_rollout_spec *spec, float *d_rec_logp, float *d_rec_value) {
    if (!h || !spec || spec->struct_size != sizeof *spec) return GYMNET_ERR_INVALID_ARG;
    if ((d_rec_logp || d_rec_value) && spec->action_source != GYMNET_ACTIONS_ACTOR) return GYMNET_ERR_INVALID_ARG;
    if (d_rec_value && !g_last.has_critic) return GYMNET_ERR_INVALID_ARG;
    if (spec->steps < 0) return GYMNET_ERR_INVALID_ARG;
    logged(VALUE_STUB_ROLLOUT);
    if (!d_rec_value) g_last.forwarded += 1;
    g_last.steps = spec->steps; g_last.action_source = spec->action_source;
    g_last.epsilon = spec->epsilon; g_last.seed = spec->action_seed; g_last.tick = spec->action_tick0;
    for (int64_t k = 0; k < spec->steps * g_lanes; ++k) {
        if (d_rec_logp) d_rec_logp[k] = -(float)k;
        if (d_rec_value) d_rec_value[k] = (float)k;
        if (spec->d_rec_actions) ((int32_t *)spec->d_rec_actions)[k] = (int32_t)(k & 1);
    }
    return GYMNET_OK;
}
