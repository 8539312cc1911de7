/* tests/cpp/advantage_stub.c — TEST-ONLY stand-in for gymnet_gae_device, linked beside tests/cpp/abi_stub.c (which has the rest of the C
 * ABI) for the sanitizer build of tests/cpp/advantage_test.cpp.  It runs the header's recurrence on HOST memory and touches exactly the
 * elements the contract names: it READS d_reward[t * stride + i], d_done[..], d_value[..], d_boot[..] for t < steps, i < count and
 * d_last_value[i], and WRITES d_advantage / d_return at the same offsets — so a size or stride the C++ side got wrong is an
 * out-of-bounds access the sanitizer sees.  It refuses what the header says the library refuses.  The product never links it. */
#include <math.h>
#include <stddef.h>

#include "gymnet_amd.h"

typedef struct advantage_stub_call {
    int calls, device;
    void *stream;
    int64_t steps, count, stride;
    float gamma, lambda;
} advantage_stub_call;

static advantage_stub_call g_last;

const advantage_stub_call *advantage_stub_last(void) { return &g_last; }

int gymnet_gae_device(int device, void *stream, int64_t steps, int64_t count, int64_t stride, const float *d_reward, const uint8_t *d_done,
                      const float *d_value, const float *d_last_value, const float *d_boot, float gamma, float lambda, float *d_advantage,
                      float *d_return) {
    if (steps < 0 || count < 0 || stride < count) return GYMNET_ERR_INVALID_ARG;
    if (!(gamma >= 0.0f && gamma <= 1.0f) || !(lambda >= 0.0f && lambda <= 1.0f)) return GYMNET_ERR_INVALID_ARG;
    if (!d_reward || !d_done || (!d_advantage && !d_return)) return GYMNET_ERR_INVALID_ARG;
    if (d_advantage == d_return) return GYMNET_ERR_INVALID_ARG;
    const float *outs[2] = {d_advantage, d_return};
    for (int k = 0; k < 2; ++k)
        if (outs[k] && ((const void *)outs[k] == (const void *)d_done || outs[k] == d_boot || outs[k] == d_last_value)) return GYMNET_ERR_INVALID_ARG;
    g_last.calls += 1; g_last.device = device; g_last.stream = stream;
    g_last.steps = steps; g_last.count = count; g_last.stride = stride; g_last.gamma = gamma; g_last.lambda = lambda;
    const float gl = gamma * lambda;
    for (int64_t i = 0; i < count; ++i) {
        float A = 0.0f, vnext = d_last_value ? d_last_value[i] : 0.0f;
        for (int64_t t = steps - 1; t >= 0; --t) {
            const int64_t k = t * stride + i;
            const uint8_t d = d_done[k];
            const float r = d_reward[k], v = d_value ? d_value[k] : 0.0f, b = d_boot ? d_boot[k] : 0.0f;
            const float nv = (d & 1) ? 0.0f : (d & 2) ? b : vnext;
            const float delta = fmaf(gamma, nv, r) - v;
            A = d ? delta : fmaf(gl, A, delta);
            if (d_advantage) d_advantage[k] = A;
            if (d_return) d_return[k] = A + v;
            vnext = v;
        }
    }
    return GYMNET_OK;
}
