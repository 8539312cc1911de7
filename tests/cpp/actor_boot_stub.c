/* tests/cpp/actor_boot_stub.c — TEST-ONLY stand-ins for the three boot calls (gymnet_vecenv_actor_boot_device,
 * gymnet_vecenv_rollout_fused_value_boot_device, gymnet_vecenv_rollout_fused_box_boot_device), linked beside tests/cpp/abi_stub.c (which
 * has the rest of the C ABI) for the sanitizer build of tests/cpp/actor_boot_test.cpp, and built alone as a shared library that
 * tests/test_actor_boot_host.py hands to the Python wrapper in the library's place.  Like abi_stub.c they touch exactly what the header
 * documents, on HOST memory: boot WRITES num_envs floats; a rollout steps * num_envs floats of d_rec_value and of d_rec_boot and, where
 * given, as many of d_rec_logp / d_rec_logd — so a buffer sized short is an out-of-bounds write the sanitizer sees.  A NULL d_rec_boot
 * counts as a forward to the call without it.  The stub has no actor: every handle counts as one with an actor of the kind the call
 * serves, with a critic and a time limit as boot_stub_setup says, and a boot is accepted while boot_stub_stepped() has been called since
 * the last boot_stub_pushed().  Every call is appended to a log of call ids.  The product never links it. */
#include <stddef.h>

#include "gymnet_amd.h"

enum { BOOT_STUB_BOOT = 1, BOOT_STUB_VALUE_ROLLOUT = 2, BOOT_STUB_BOX_ROLLOUT = 3 };

typedef struct boot_stub_call {
    int calls, forwarded;
    int log[16];                               /* the ids of the first 16 calls, in order */
    float epsilon; uint64_t seed, tick;
    int64_t steps; int32_t action_source;
    const float *lp_at, *value_at, *boot_at;   /* the pointers of the last call */
} boot_stub_call;

static boot_stub_call g_last;
static int64_t g_lanes = 0;
static int g_critic = 0, g_limit = 0, g_stepped = 0;

const boot_stub_call *boot_stub_last(void) { return &g_last; }
void boot_stub_setup(int64_t n, int critic, int max_episode_steps) { g_lanes = n; g_critic = critic; g_limit = max_episode_steps; }
void boot_stub_clear(void) { boot_stub_call zero = {0}; g_last = zero; g_stepped = 0; }
void boot_stub_stepped(void) { g_stepped = 1; }
void boot_stub_pushed(void) { g_stepped = 0; }

static void logged(int id) {
    if (g_last.calls < 16) g_last.log[g_last.calls] = id;
    g_last.calls += 1;
}

int gymnet_vecenv_actor_boot_device(gymnet_vecenv *h, float *d_boot) {
    if (!h || !g_critic || !d_boot || ((uintptr_t)d_boot & 3u) || !g_stepped || g_limit == 0) return GYMNET_ERR_INVALID_ARG;
    logged(BOOT_STUB_BOOT);
    g_last.boot_at = d_boot;
    for (int64_t i = 0; i < g_lanes; ++i) d_boot[i] = (i & 1) ? 2000.0f + (float)i : 0.0f;
    return GYMNET_OK;
}

static int rollout(int id, gymnet_vecenv *h, const gymnet_rollout_spec *spec, float *d_rec_lp, float *d_rec_value, float *d_rec_boot) {
    if (!h || !spec || spec->struct_size != sizeof *spec) return GYMNET_ERR_INVALID_ARG;
    if (d_rec_boot && !d_rec_value) return GYMNET_ERR_INVALID_ARG;
    if ((d_rec_lp || d_rec_value) && spec->action_source != GYMNET_ACTIONS_ACTOR) return GYMNET_ERR_INVALID_ARG;
    if (d_rec_value && !g_critic) return GYMNET_ERR_INVALID_ARG;
    if (d_rec_boot && (g_limit == 0 || ((uintptr_t)d_rec_boot & 3u))) return GYMNET_ERR_INVALID_ARG;
    if (spec->steps < 0) return GYMNET_ERR_INVALID_ARG;
    logged(id);
    if (!d_rec_boot) g_last.forwarded += 1;
    g_last.steps = spec->steps; g_last.action_source = spec->action_source;
    g_last.epsilon = spec->epsilon; g_last.seed = spec->action_seed; g_last.tick = spec->action_tick0;
    g_last.lp_at = d_rec_lp; g_last.value_at = d_rec_value; g_last.boot_at = d_rec_boot;
    for (int64_t k = 0; k < spec->steps * g_lanes; ++k) {
        if (d_rec_lp) d_rec_lp[k] = -(float)k;
        if (d_rec_value) d_rec_value[k] = (float)k;
        if (d_rec_boot) d_rec_boot[k] = (k & 1) ? 2000.0f + (float)k : 0.0f;
    }
    return GYMNET_OK;
}

int gymnet_vecenv_rollout_fused_value_boot_device(gymnet_vecenv *h, const gymnet_rollout_spec *spec, float *d_rec_logp, float *d_rec_value,
                                                  float *d_rec_boot) {
    return rollout(BOOT_STUB_VALUE_ROLLOUT, h, spec, d_rec_logp, d_rec_value, d_rec_boot);
}

int gymnet_vecenv_rollout_fused_box_boot_device(gymnet_vecenv *h, const gymnet_rollout_spec *spec, float *d_rec_logd, float *d_rec_value,
                                                float *d_rec_boot) {
    return rollout(BOOT_STUB_BOX_ROLLOUT, h, spec, d_rec_logd, d_rec_value, d_rec_boot);
}
