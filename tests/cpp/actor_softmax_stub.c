/* tests/cpp/actor_softmax_stub.c — TEST-ONLY stand-ins for gymnet_vecenv_actor_set_exploration and gymnet_vecenv_actor_get_exploration,
 * linked beside tests/cpp/abi_stub.c (which has the rest of the C ABI) for the sanitizer build of tests/cpp/actor_softmax_test.cpp.  Like
 * abi_stub.c they touch exactly what the header documents: set stores its two arguments after the header's argument checks, get WRITES
 * one int32 and one float through the pointers that are not NULL, and both record their calls.  The stub has no actor: every handle
 * counts as one with a Discrete actor at (UNIFORM, 1.0).  The product never links it. */
#include <math.h>
#include <stddef.h>

#include "gymnet_amd.h"

typedef struct softmax_stub_call { int sets, gets; int32_t explore; float temperature; } softmax_stub_call;

static softmax_stub_call g_last = {0, 0, GYMNET_ACTOR_EXPLORE_UNIFORM, 1.0f};

const softmax_stub_call *softmax_stub_last(void) { return &g_last; }

int gymnet_vecenv_actor_set_exploration(gymnet_vecenv *h, int32_t explore, float temperature) {
    if (!h) return GYMNET_ERR_INVALID_ARG;
    if (explore != GYMNET_ACTOR_EXPLORE_UNIFORM && explore != GYMNET_ACTOR_EXPLORE_SOFTMAX) return GYMNET_ERR_INVALID_ARG;
    if (!(isfinite(temperature) && temperature > 0.0f && isfinite(1.0f / temperature))) return GYMNET_ERR_INVALID_ARG;
    g_last.sets += 1;
    g_last.explore = explore; g_last.temperature = temperature;
    return GYMNET_OK;
}

int gymnet_vecenv_actor_get_exploration(gymnet_vecenv *h, int32_t *explore, float *temperature) {
    if (!h) return GYMNET_ERR_INVALID_ARG;
    g_last.gets += 1;
    if (explore) *explore = g_last.explore;
    if (temperature) *temperature = g_last.temperature;
    return GYMNET_OK;
}
