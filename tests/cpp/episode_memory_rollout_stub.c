/* tests/cpp/episode_memory_rollout_stub.c — TEST-ONLY stand-ins for gymnet_vecenv_memory_config_rollout and
 * gymnet_vecenv_memory_push_rollout_device, linked beside tests/cpp/abi_stub.c (which has the rest of the C ABI) for the sanitizer build of
 * tests/cpp/episode_memory_rollout_test.cpp.  Like abi_stub.c they touch exactly the bytes the header documents: the ingest READS
 * rec_obs [steps][obs_dim][n] floats, reward [steps][n] floats, done [steps][n] bytes and the action rows (t % ring) * action_stride of n
 * 4-byte words each, for the shape the test announced with rollout_stub_shape, and records its arguments.  The product never links it. */
#include <stddef.h>
#include <string.h>

#include "gymnet_amd.h"

typedef struct rollout_stub_call {
    int calls;
    int32_t capacity, max_length, history, rollout_chunk;
    int64_t steps, action_stride, ring;
    const void *rec_obs, *actions, *rec_reward, *rec_done;
} rollout_stub_call;

static rollout_stub_call g_last;
static int64_t g_n;
static int g_obs_dim;
static volatile unsigned char g_sink;

static void read_all(const void *p, size_t bytes) {
    const unsigned char *b = (const unsigned char *)p;
    unsigned char s = 0;
    for (size_t i = 0; i < bytes; ++i) s ^= b[i];
    g_sink = s;
}

void rollout_stub_shape(int64_t n, int obs_dim) { g_n = n; g_obs_dim = obs_dim; }
const rollout_stub_call *rollout_stub_last(void) { return &g_last; }

int gymnet_vecenv_memory_config_rollout(gymnet_vecenv *h, int32_t capacity, int32_t max_length, int32_t history, int32_t rollout_chunk) {
    if (!h || rollout_chunk < 1 || rollout_chunk > 64) return GYMNET_ERR_INVALID_ARG;
    g_last.calls += 1;
    g_last.capacity = capacity; g_last.max_length = max_length; g_last.history = history; g_last.rollout_chunk = rollout_chunk;
    return GYMNET_OK;
}

int gymnet_vecenv_memory_push_rollout_device(gymnet_vecenv *h, int64_t steps, const void *d_rec_obs, const void *d_actions,
                                             int64_t action_stride, int64_t ring, const float *d_rec_reward, const uint8_t *d_rec_done) {
    if (!h || !d_rec_obs || !d_actions || !d_rec_reward || !d_rec_done || steps < 1 || ring < 1 || action_stride < 0) return GYMNET_ERR_INVALID_ARG;
    read_all(d_rec_obs, (size_t)steps * (size_t)g_obs_dim * (size_t)g_n * 4);
    read_all(d_rec_reward, (size_t)steps * (size_t)g_n * 4);
    read_all(d_rec_done, (size_t)steps * (size_t)g_n);
    for (int64_t t = 0; t < steps; ++t) read_all((const char *)d_actions + (size_t)((t % ring) * action_stride) * 4, (size_t)g_n * 4);
    g_last.calls += 1;
    g_last.steps = steps; g_last.action_stride = action_stride; g_last.ring = ring;
    g_last.rec_obs = d_rec_obs; g_last.actions = d_actions; g_last.rec_reward = d_rec_reward; g_last.rec_done = d_rec_done;
    return GYMNET_OK;
}
