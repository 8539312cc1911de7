// actor_box_test.cpp — the C++ host side of the Box actor (gymnet::VectorEnv::ConfigureBoxActor / BoxActorAct in
// include/gymnet_amd.hpp), built with g++ against libgymnet_amd.so and the HIP runtime.
//   --cpu: the two calls refuse a null handle and write nothing; no GPU needed.
//   --gpu: a Pendulum handle with the one-layer net [3, 1] whose weights are (0, 0, -k): the actions equal clamp(-k * theta_dot) of the
//          newest observation (k is large enough that lanes land on both bounds and inside), and a stale act is refused.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <string>
#include <vector>

#include "gymnet_amd.hpp"

static int failed = 0;
#define CHECK(cond, msg)                                                          \
    do {                                                                          \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, msg); ++failed; } \
    } while (0)

static void cpu_checks() {
    int32_t widths[2] = {3, 1};
    float w[4] = {0, 0, -1, 0};
    float out[2] = {-7.0f, -7.0f};
    CHECK(gymnet_vecenv_actor_box_config(nullptr, 1, 1, widths, w, 4) == GYMNET_ERR_INVALID_ARG, "box_config");
    CHECK(gymnet_vecenv_actor_box_act_device(nullptr, &out[0], &out[1], 0.0f, 0, 0) == GYMNET_ERR_INVALID_ARG, "box_act");
    CHECK(widths[0] == 3 && widths[1] == 1 && out[0] == -7.0f && out[1] == -7.0f, "nothing written");
}

static void gpu_checks() {
    const int64_t n = 1000;
    const float k = 2.0f;
    gymnet::VectorEnv env(GYMNET_ENV_PENDULUM, n, 0, 7, 0);
    env.Reset();
    env.ConfigureBoxActor(1, {3, 1}, {0.0f, 0.0f, -k, 0.0f});
    float *d_act = nullptr, *d_raw = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_act), sizeof(float) * n) == hipSuccess, "hipMalloc");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_raw), sizeof(float) * n) == hipSuccess, "hipMalloc");
    for (int t = 0; t < 20; ++t) {
        env.BoxActorAct(d_act);
        env.StepDevice(d_act);
        env.PushActor();
    }
    env.BoxActorAct(d_act, 0.0f, 0, 0, d_raw);
    gymnet::check(gymnet_vecenv_sync(env.handle()));          // the copies below are not ordered after the handle's stream
    std::vector<float> act((size_t)n), raw((size_t)n), st((size_t)(2 * n));
    CHECK(hipMemcpy(act.data(), d_act, sizeof(float) * n, hipMemcpyDeviceToHost) == hipSuccess, "copy");
    CHECK(hipMemcpy(raw.data(), d_raw, sizeof(float) * n, hipMemcpyDeviceToHost) == hipSuccess, "copy");
    gymnet::check(gymnet_vecenv_get_state(env.handle(), st.data()));
    bool rule = true, unclamped = true;
    int low = 0, high = 0, inside = 0;
    for (int64_t i = 0; i < n; ++i) {
        const float r = -k * st[(size_t)(n + i)];             // one product, no sum to round: exact in the kernel's fmaf(w, x, +0) chain
        const float want = r < -2.0f ? -2.0f : (r > 2.0f ? 2.0f : r);
        rule &= act[(size_t)i] == want;
        unclamped &= raw[(size_t)i] == r;
        low += want == -2.0f; high += want == 2.0f; inside += want > -2.0f && want < 2.0f;
    }
    CHECK(rule, "the actions are clamp(-k * theta_dot)");
    CHECK(unclamped, "d_raw holds the unclamped outputs");
    CHECK(low > 0 && high > 0 && inside > 0, "lanes on both bounds and inside");
    env.StepDevice(d_act);
    bool refused = false;
    try { env.BoxActorAct(d_act); } catch (const std::exception &) { refused = true; }
    CHECK(refused, "a stale act is refused");
    env.PushActor();
    env.BoxActorAct(d_act);
    env.ConfigureBoxActor(0, {}, {});
    (void)hipFree(d_act);
    (void)hipFree(d_raw);
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::string(argv[1]) == "--gpu";
    cpu_checks();
    if (gpu) gpu_checks();
    std::printf("%s: %d failed\n", gpu ? "cpu+gpu" : "cpu", failed);
    return failed ? 1 : 0;
}
