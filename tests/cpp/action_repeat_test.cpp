// action_repeat_test.cpp — the C++ host side of frame skip (gymnet::VectorEnv::StepRepeatDevice / StepRepeatInto / RolloutRepeatDevice in
// include/gymnet_amd.hpp), built with g++ against libgymnet_amd.so and the HIP runtime.
//   --cpu: the three calls refuse a null handle and write nothing; no GPU needed.
//   --gpu: two MountainCar handles of 64 lanes with one seed: StepRepeatDevice(actions, 2) — R = 3 — on one equals three StepDevice calls
//          on the other for the lanes that did not finish (MountainCar needs ~100 steps to the goal: none does), and the tick moved by 3.
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
    int32_t actions[2] = {1, 2};
    float obs[4] = {-7.0f, -7.0f, -7.0f, -7.0f}, reward[2] = {-7.0f, -7.0f};
    uint8_t done[2] = {9, 9};
    gymnet_rollout_spec spec{};
    spec.struct_size = (uint32_t)sizeof spec;
    CHECK(gymnet_vecenv_step_repeat_device(nullptr, actions, 1) == GYMNET_ERR_INVALID_ARG, "step_repeat_device");
    CHECK(gymnet_vecenv_step_repeat(nullptr, actions, 1, obs, reward, done) == GYMNET_ERR_INVALID_ARG, "step_repeat");
    CHECK(gymnet_vecenv_rollout_repeat_device(nullptr, &spec, 1) == GYMNET_ERR_INVALID_ARG, "rollout_repeat_device");
    CHECK(obs[0] == -7.0f && obs[3] == -7.0f && reward[0] == -7.0f && reward[1] == -7.0f && done[0] == 9 && done[1] == 9, "nothing written");
}

static void gpu_checks() {
    const int64_t n = 64;
    gymnet::VectorEnv held(GYMNET_ENV_MOUNTAINCAR, n, 0, 11, 0), single(GYMNET_ENV_MOUNTAINCAR, n, 0, 11, 0);
    held.Reset();
    single.Reset();
    std::vector<int32_t> a((size_t)n);
    for (int64_t i = 0; i < n; ++i) a[(size_t)i] = (int32_t)(i % 3);
    int32_t *d_act = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_act), sizeof(int32_t) * n) == hipSuccess, "hipMalloc");
    CHECK(hipMemcpy(d_act, a.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice) == hipSuccess, "copy");
    uint64_t t0 = 0, t1 = 0, ts = 0;
    gymnet::check(gymnet_vecenv_get_tick(held.handle(), &t0));
    held.StepRepeatDevice(d_act, 2);
    for (int k = 0; k < 3; ++k) single.StepDevice(d_act);
    held.Sync();
    single.Sync();
    gymnet::check(gymnet_vecenv_get_tick(held.handle(), &t1));
    gymnet::check(gymnet_vecenv_get_tick(single.handle(), &ts));
    CHECK(t1 == t0 + 3 && t1 == ts, "the tick moved by 3");
    const std::vector<float> sh = held.GetState(), ss = single.GetState();
    std::vector<float> rh((size_t)n), rs((size_t)n), oh((size_t)(2 * n)), os((size_t)(2 * n));
    std::vector<uint8_t> dh((size_t)n), ds((size_t)n);
    gymnet::check(gymnet_vecenv_read(held.handle(), oh.data(), rh.data(), dh.data()));
    gymnet::check(gymnet_vecenv_read(single.handle(), os.data(), rs.data(), ds.data()));
    bool same = true, summed = true;
    int unfinished = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (dh[(size_t)i]) continue;
        ++unfinished;
        same &= sh[(size_t)i] == ss[(size_t)i] && sh[(size_t)(n + i)] == ss[(size_t)(n + i)] && ds[(size_t)i] == 0;
        same &= oh[(size_t)(2 * i)] == os[(size_t)(2 * i)] && oh[(size_t)(2 * i + 1)] == os[(size_t)(2 * i + 1)];
        summed &= rh[(size_t)i] == -3.0f && rs[(size_t)i] == -1.0f;      // (-1 + -1) + -1 against the last single step's -1
    }
    CHECK(unfinished == n, "no lane reaches the goal in three steps");
    CHECK(same, "StepRepeatDevice(actions, 2) equals three StepDevice calls");
    CHECK(summed, "the decision's reward is the sum of its three sub-steps");
    bool refused = false;
    try { held.StepRepeatDevice(d_act, 256); } catch (const std::exception &) { refused = true; }
    CHECK(refused, "repeat = 256 is refused");
    (void)hipFree(d_act);
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::string(argv[1]) == "--gpu";
    cpu_checks();
    if (gpu) gpu_checks();
    std::printf("%s: %d failed\n", gpu ? "cpu+gpu" : "cpu", failed);
    return failed ? 1 : 0;
}
