// actor_test.cpp — the C++ host side of the actor (gymnet::VectorEnv::ConfigureActor / ActorAct / PushActor / ResetActor /
// LoadActorWeights in include/gymnet_amd.hpp), built with g++ against libgymnet_amd.so and the HIP runtime.
//   --cpu: the calls refuse a null handle and write nothing; no GPU needed.
//   --gpu: a CartPole auto-reset handle with a one-layer actor whose weights pick action 1 exactly where the pole leans right
//          (x[2] > 0 of the newest observation): the actions equal that rule, a stale act is refused, and LoadActorWeights with the
//          negated weights flips every action whose logit is not zero.
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
    int32_t widths[2] = {4, 2};
    float w[10] = {};
    float *hist = reinterpret_cast<float *>(&w[0]);
    int64_t stride = -7;
    int32_t slot = -7;
    CHECK(gymnet_vecenv_actor_config(nullptr, 1, 1, widths, w, 10) == GYMNET_ERR_INVALID_ARG, "config");
    CHECK(gymnet_vecenv_actor_load_device(nullptr, w, 10) == GYMNET_ERR_INVALID_ARG, "load");
    CHECK(gymnet_vecenv_actor_reset_device(nullptr, nullptr) == GYMNET_ERR_INVALID_ARG, "reset");
    CHECK(gymnet_vecenv_actor_push_device(nullptr, nullptr) == GYMNET_ERR_INVALID_ARG, "push");
    CHECK(gymnet_vecenv_actor_act_device(nullptr, widths, nullptr, 0.0f, 0, 0) == GYMNET_ERR_INVALID_ARG, "act");
    CHECK(gymnet_vecenv_actor_view(nullptr, &hist, &stride, &slot) == GYMNET_ERR_INVALID_ARG, "view");
    CHECK(widths[0] == 4 && widths[1] == 2 && stride == -7 && slot == -7 && hist == &w[0], "nothing written");
}

static void gpu_checks() {
    const int64_t n = 1000;
    gymnet::VectorEnv env(GYMNET_ENV_CARTPOLE, n, 0, 7, GYMNET_FLAG_AUTORESET);
    env.Reset();
    // logit 0 = 0, logit 1 = x[2]: action 1 where the angle is > 0
    std::vector<float> weights = {0, 0, 0, 0, 0, 0, 1, 0, 0, 0};
    env.ConfigureActor(1, {4, 2}, weights);
    int32_t *d_act = nullptr;
    float *d_w = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_act), sizeof(int32_t) * n) == hipSuccess, "hipMalloc");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_w), sizeof(float) * weights.size()) == hipSuccess, "hipMalloc");
    std::vector<int32_t> act((size_t)n);
    for (int t = 0; t < 20; ++t) {
        env.ActorAct(d_act);
        env.StepDevice(d_act);
        env.PushActor();
    }
    env.ActorAct(d_act);
    gymnet::check(gymnet_vecenv_sync(env.handle()));          // the copy below is not ordered after the handle's stream
    CHECK(hipMemcpy(act.data(), d_act, sizeof(int32_t) * n, hipMemcpyDeviceToHost) == hipSuccess, "copy");
    std::vector<float> st((size_t)(4 * n));
    gymnet::check(gymnet_vecenv_get_state(env.handle(), st.data()));
    bool rule = true;
    for (int64_t k = 0; k < n; ++k) rule &= act[(size_t)k] == (st[(size_t)(2 * n + k)] > 0.0f ? 1 : 0);
    CHECK(rule, "the actions follow the weights");
    env.StepDevice(d_act);
    bool refused = false;
    try { env.ActorAct(d_act); } catch (const std::exception &) { refused = true; }
    CHECK(refused, "a stale act is refused");
    env.PushActor();
    std::vector<float> neg = weights;
    for (float &v : neg) v = -v;
    CHECK(hipMemcpy(d_w, neg.data(), sizeof(float) * neg.size(), hipMemcpyHostToDevice) == hipSuccess, "copy");
    env.LoadActorWeights(d_w, (int64_t)neg.size());
    env.ActorAct(d_act);
    gymnet::check(gymnet_vecenv_sync(env.handle()));          // the copy below is not ordered after the handle's stream
    CHECK(hipMemcpy(act.data(), d_act, sizeof(int32_t) * n, hipMemcpyDeviceToHost) == hipSuccess, "copy");
    gymnet::check(gymnet_vecenv_get_state(env.handle(), st.data()));
    bool flipped = true;
    for (int64_t k = 0; k < n; ++k) flipped &= act[(size_t)k] == (st[(size_t)(2 * n + k)] < 0.0f ? 1 : 0);
    CHECK(flipped, "LoadActorWeights: negated weights");
    env.ConfigureActor(0, {}, {});
    (void)hipFree(d_act);
    (void)hipFree(d_w);
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::string(argv[1]) == "--gpu";
    cpu_checks();
    if (gpu) gpu_checks();
    std::printf("%s: %d failed\n", gpu ? "cpu+gpu" : "cpu", failed);
    return failed ? 1 : 0;
}
