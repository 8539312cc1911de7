// actor_box_policy_test.cpp — the C++ host side of a Box actor's policy (gymnet::VectorEnv::SetBoxActorPolicy / GetBoxActorPolicy in
// include/gymnet_amd.hpp), built with g++ against libgymnet_amd.so and the HIP runtime.
//   --cpu: the two calls refuse a null handle and write nothing; on a machine without a GPU the handle a policy would belong to is
//          refused with NO_DEVICE (NoDeviceError), so no compute call gets further than that; no GPU needed.
//   --gpu: a Pendulum handle with the one-layer net [3, 1] whose weights are (0, 0, -k): raw = -k * theta_dot.  Under (TANH, SAMPLE) the
//          greedy actions are 2 * tanh(raw) within the header's bound; under (TANH, GAUSSIAN, 0) with epsilon 1 they are the same values;
//          with sigma 0.5 most lanes leave them and stay inside the bounds; the policy round-trips, bad arguments are refused and leave it,
//          and a re-config returns it to the default.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "gymnet_amd.hpp"

static int failed = 0;
#define CHECK(cond, msg)                                                          \
    do {                                                                          \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, msg); ++failed; } \
    } while (0)

static void cpu_checks(bool gpu) {
    int32_t head = -9, explore = -9;
    float sigma = -9.0f;
    CHECK(gymnet_vecenv_actor_box_set_policy(nullptr, GYMNET_BOX_HEAD_TANH, GYMNET_BOX_EXPLORE_GAUSSIAN, 0.5f) == GYMNET_ERR_INVALID_ARG, "set_policy");
    CHECK(gymnet_vecenv_actor_box_get_policy(nullptr, &head, &explore, &sigma) == GYMNET_ERR_INVALID_ARG, "get_policy");
    CHECK(head == -9 && explore == -9 && sigma == -9.0f, "nothing written");
    CHECK(GYMNET_BOX_HEAD_CLAMP == 0 && GYMNET_BOX_HEAD_TANH == 1 && GYMNET_BOX_EXPLORE_SAMPLE == 0 && GYMNET_BOX_EXPLORE_GAUSSIAN == 1, "enum values");
    CHECK(GYMNET_ABI_VERSION == 6, "ABI 6");
    int ndev = 0;
    if (!gpu && gymnet_device_count(&ndev) != GYMNET_OK) {
        // no GPU here: the engine refuses loudly, a policy never reaches a CPU path
        CHECK(ndev == 0, "count reported as 0");
        bool no_device = false;
        try { gymnet::VectorEnv e(GYMNET_ENV_PENDULUM, 16); } catch (const gymnet::NoDeviceError &) { no_device = true; }
        CHECK(no_device, "no device -> NoDeviceError");
    }
}

static std::vector<float> act(gymnet::VectorEnv &env, float *d_act, float *d_raw, float epsilon, int64_t n, std::vector<float> *raw = nullptr) {
    env.BoxActorAct(d_act, epsilon, 5, 3, d_raw);
    gymnet::check(gymnet_vecenv_sync(env.handle()));
    std::vector<float> out((size_t)n);
    CHECK(hipMemcpy(out.data(), d_act, sizeof(float) * n, hipMemcpyDeviceToHost) == hipSuccess, "copy");
    if (raw) {
        raw->resize((size_t)n);
        CHECK(hipMemcpy(raw->data(), d_raw, sizeof(float) * n, hipMemcpyDeviceToHost) == hipSuccess, "copy");
    }
    return out;
}

static void gpu_checks() {
    const int64_t n = 321;
    const float k = 4.0f;                                      // theta_dot starts in [-1, 1]: outputs on both sides of the bounds
    gymnet::VectorEnv env(GYMNET_ENV_PENDULUM, n, 0, 7, 0);
    env.Reset();
    env.ConfigureBoxActor(1, {3, 1}, {0.0f, 0.0f, -k, 0.0f});
    gymnet_box_head head = GYMNET_BOX_HEAD_TANH;
    gymnet_box_explore explore = GYMNET_BOX_EXPLORE_GAUSSIAN;
    float sigma = -1.0f;
    env.GetBoxActorPolicy(head, explore, sigma);
    CHECK(head == GYMNET_BOX_HEAD_CLAMP && explore == GYMNET_BOX_EXPLORE_SAMPLE && sigma == 0.0f, "a new actor has the default policy");
    float *d_act = nullptr, *d_raw = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_act), sizeof(float) * n) == hipSuccess, "hipMalloc");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_raw), sizeof(float) * n) == hipSuccess, "hipMalloc");

    env.SetBoxActorPolicy(GYMNET_BOX_HEAD_TANH, GYMNET_BOX_EXPLORE_SAMPLE, 0.75f);
    env.GetBoxActorPolicy(head, explore, sigma);
    CHECK(head == GYMNET_BOX_HEAD_TANH && explore == GYMNET_BOX_EXPLORE_SAMPLE && sigma == 0.75f, "round trip; sigma is stored whatever explore is");
    std::vector<float> raw, st((size_t)(2 * n));
    const std::vector<float> greedy = act(env, d_act, d_raw, 0.0f, n, &raw);
    gymnet::check(gymnet_vecenv_get_state(env.handle(), st.data()));
    // the header's bound for the tanh greedy: half * 5 * 2^-24 plus one spacing of float32(2)
    const double bound = 2.0 * 5.0 * std::ldexp(1.0, -24) + std::ldexp(1.0, -22);
    bool rule = true, unchanged = true;
    int saturated = 0, inside = 0;
    for (int64_t i = 0; i < n; ++i) {
        const float r = -k * st[(size_t)(n + i)];             // one product, no sum to round: exact in the kernel's fmaf(w, x, +0) chain
        unchanged &= raw[(size_t)i] == r;
        rule &= std::fabs((double)greedy[(size_t)i] - 2.0 * std::tanh((double)r)) <= bound && std::fabs(greedy[(size_t)i]) <= 2.0f;
        saturated += std::fabs(r) > 2.0f; inside += std::fabs(r) <= 2.0f;
    }
    CHECK(rule, "the greedy actions are 2 * tanh(-k * theta_dot)");
    CHECK(unchanged, "d_raw holds the network's outputs, unchanged");
    CHECK(saturated > 0 && inside > 0, "outputs beyond the bounds and inside");

    env.SetBoxActorPolicy(GYMNET_BOX_HEAD_TANH, GYMNET_BOX_EXPLORE_GAUSSIAN, 0.0f);
    const std::vector<float> still = act(env, d_act, d_raw, 1.0f, n);
    bool same = true;
    for (int64_t i = 0; i < n; ++i) same &= still[(size_t)i] == greedy[(size_t)i];
    CHECK(same, "sigma 0: every exploring lane keeps its greedy value");
    env.SetBoxActorPolicy(GYMNET_BOX_HEAD_TANH, GYMNET_BOX_EXPLORE_GAUSSIAN, 0.5f);
    const std::vector<float> noisy = act(env, d_act, d_raw, 1.0f, n);
    int moved = 0;
    bool bounded = true;
    for (int64_t i = 0; i < n; ++i) {
        moved += noisy[(size_t)i] != greedy[(size_t)i];
        bounded &= noisy[(size_t)i] >= -2.0f && noisy[(size_t)i] <= 2.0f && std::fabs(noisy[(size_t)i] - greedy[(size_t)i]) <= 0.5f * 5.78f;
    }
    CHECK(moved > n / 2, "sigma 0.5: the exploring lanes leave the greedy action");
    CHECK(bounded, "... by at most sigma * |z|, and stay inside the bounds");

    const float bad_sigma[3] = {std::numeric_limits<float>::quiet_NaN(), -1.0f, std::numeric_limits<float>::infinity()};
    for (float s : bad_sigma) CHECK(gymnet_vecenv_actor_box_set_policy(env.handle(), 1, 1, s) == GYMNET_ERR_INVALID_ARG, "sigma");
    CHECK(gymnet_vecenv_actor_box_set_policy(env.handle(), 2, 1, 0.5f) == GYMNET_ERR_INVALID_ARG, "head");
    CHECK(gymnet_vecenv_actor_box_set_policy(env.handle(), 1, -1, 0.5f) == GYMNET_ERR_INVALID_ARG, "explore");
    bool refused = false;
    try { env.SetBoxActorPolicy((gymnet_box_head)7, GYMNET_BOX_EXPLORE_SAMPLE); } catch (const std::exception &) { refused = true; }
    CHECK(refused, "the wrapper throws on a refusal");
    env.GetBoxActorPolicy(head, explore, sigma);
    CHECK(head == GYMNET_BOX_HEAD_TANH && explore == GYMNET_BOX_EXPLORE_GAUSSIAN && sigma == 0.5f, "refusals leave the policy");

    env.StepDevice(d_act);                                      // the fused rollout's unfused counterpart accepts the policy's actions
    env.PushActor();
    env.GetBoxActorPolicy(head, explore, sigma);
    CHECK(head == GYMNET_BOX_HEAD_TANH && sigma == 0.5f, "a push keeps the policy");
    env.ConfigureBoxActor(1, {3, 1}, {0.0f, 0.0f, -k, 0.0f});
    env.GetBoxActorPolicy(head, explore, sigma);
    CHECK(head == GYMNET_BOX_HEAD_CLAMP && explore == GYMNET_BOX_EXPLORE_SAMPLE && sigma == 0.0f, "a re-config returns to the default");
    env.ConfigureBoxActor(0, {}, {});
    (void)hipFree(d_act);
    (void)hipFree(d_raw);
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::string(argv[1]) == "--gpu";
    cpu_checks(gpu);
    if (gpu) gpu_checks();
    std::printf("%s: %d failed\n", gpu ? "cpu+gpu" : "cpu", failed);
    return failed ? 1 : 0;
}
