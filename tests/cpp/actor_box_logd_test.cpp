// actor_box_logd_test.cpp — the C++ host side of the Box actor's log-density (gymnet::VectorEnv::BoxActorActLogd / RolloutFusedBoxLogd in
// include/gymnet_amd.hpp).
//   --stub: built with -DLOGD_STUB against tests/cpp/abi_stub.c and tests/cpp/actor_box_logd_stub.c, under the sanitizers: the two methods
//           hand their arguments across unchanged into buffers of exactly the documented sizes, set struct_size, forward on null
//           pointers, and throw on a refusal.
//   --cpu:  built against libgymnet_amd.so: the two calls refuse a null handle and write nothing; no GPU needed.
//   --gpu:  a Pendulum handle, 321 lanes, a one-layer Box actor [3, 1] whose output is the constant 0.25 (zero weights, the bias decides)
//           under ("clamp", "gaussian", 0.5) and a one-layer critic whose value is 2.25: at epsilon = 0 every lane takes 0.25 and its
//           log-density is c = (float)(-log(0.5) - ln(2 pi) / 2) exactly, in the act call and in every row of the fused rollout, whose
//           values are 2.25; the row after the last step stays; a fresh policy (sigma 0) and a Discrete actor are refused.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gymnet_amd.hpp"

static int failed = 0;
#define CHECK(cond, msg)                                                          \
    do {                                                                          \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, msg); ++failed; } \
    } while (0)

#ifdef LOGD_STUB
extern "C" {
typedef struct logd_stub_call {
    int calls, forwarded;
    float epsilon; uint64_t seed, tick;
    int64_t steps; int32_t action_source;
    const float *logd_at, *value_at;
} logd_stub_call;
const logd_stub_call *logd_stub_last(void);
void logd_stub_setup(int64_t n, int critic);
}

static void stub_checks() {
    const int64_t n = 37, T = 3;
    gymnet::VectorEnv env(GYMNET_ENV_PENDULUM, n);
    logd_stub_setup(n, 0);
    const logd_stub_call *c = logd_stub_last();
    std::vector<float> actions((size_t)n, -7.0f), raw((size_t)n, -7.0f), logd((size_t)n, 1.0f);     // exactly the documented sizes
    env.BoxActorActLogd(actions.data(), logd.data(), 0.25f, 5, 3);
    CHECK(c->calls == 1 && c->forwarded == 0 && c->epsilon == 0.25f && c->seed == 5 && c->tick == 3 && c->logd_at == logd.data(), "arguments cross unchanged");
    CHECK(actions[n - 1] == 0.5f * (float)(n - 1) && logd[n - 1] == -(float)(n - 1) && raw[0] == -7.0f, "actions and logd written, no raw");
    env.BoxActorActLogd(actions.data(), logd.data(), 1.0f, 6, 4, raw.data());
    CHECK(c->calls == 2 && raw[n - 1] == 100.0f + (float)(n - 1), "the raw pointer crosses");
    env.BoxActorActLogd(actions.data(), logd.data());
    CHECK(c->calls == 3 && c->epsilon == 0.0f && c->seed == 0 && c->tick == 0, "the defaults are BoxActorAct's");
    std::fill(logd.begin(), logd.end(), 1.0f);
    env.BoxActorActLogd(actions.data(), nullptr, 0.5f, 1, 2);
    CHECK(c->calls == 4 && c->forwarded == 1 && logd[0] == 1.0f, "a null logd forwards");
    bool refused = false;
    try { env.BoxActorActLogd(actions.data(), logd.data(), 1.5f); } catch (const std::exception &) { refused = true; }
    CHECK(refused && c->calls == 4 && logd[0] == 1.0f, "a refusal throws and writes nothing");

    std::vector<float> rec_logd((size_t)(T * n), 1.0f), rec_value((size_t)(T * n), 1.0f), rec_act((size_t)(T * n), -7.0f);
    gymnet_rollout_spec spec{};
    spec.action_source = GYMNET_ACTIONS_ACTOR; spec.steps = T; spec.epsilon = 0.75f; spec.action_seed = 9; spec.action_tick0 = 100;
    spec.d_rec_actions = rec_act.data();
    refused = false;
    try { env.RolloutFusedBoxLogd(spec, rec_logd.data(), rec_value.data()); } catch (const std::exception &) { refused = true; }
    CHECK(refused && c->calls == 4 && rec_logd[0] == 1.0f && rec_value[0] == 1.0f, "values without a critic throw and write nothing");
    env.RolloutFusedBoxLogd(spec, rec_logd.data(), nullptr);     // (struct_size is the wrapper's to set: the stub refuses any other)
    CHECK(c->calls == 5 && c->forwarded == 1 && c->steps == T && c->action_source == GYMNET_ACTIONS_ACTOR && c->value_at == nullptr, "the spec crosses; logd alone");
    CHECK(c->epsilon == 0.75f && c->seed == 9 && c->tick == 100, "... with its action stream");
    CHECK(rec_logd[(size_t)(T * n - 1)] == -(float)(T * n - 1) && rec_act[(size_t)(T * n - 1)] == 0.5f * (float)(T * n - 1) && rec_value[0] == 1.0f, "every row written");
    logd_stub_setup(n, 1);
    std::fill(rec_logd.begin(), rec_logd.end(), 1.0f);
    env.RolloutFusedBoxLogd(spec, rec_logd.data(), rec_value.data());
    CHECK(c->calls == 6 && c->logd_at == rec_logd.data() && c->value_at == rec_value.data(), "both pointers cross, in their order");
    CHECK(rec_logd[(size_t)(T * n - 1)] == -(float)(T * n - 1) && rec_value[(size_t)(T * n - 1)] == (float)(T * n - 1), "both written");
    std::fill(rec_logd.begin(), rec_logd.end(), 1.0f);
    env.RolloutFusedBoxLogd(spec, nullptr, rec_value.data());
    CHECK(c->calls == 7 && c->forwarded == 1 && rec_logd[0] == 1.0f && c->logd_at == nullptr, "d_rec_value alone is served");
    env.RolloutFusedBoxLogd(spec, nullptr, nullptr);
    CHECK(c->calls == 8 && c->forwarded == 2, "both null forwards");
    spec.action_source = GYMNET_ACTIONS_SAMPLE;
    refused = false;
    try { env.RolloutFusedBoxLogd(spec, rec_logd.data(), nullptr); } catch (const std::exception &) { refused = true; }
    CHECK(refused && c->calls == 8 && rec_logd[0] == 1.0f, "a source other than the actor throws and writes nothing");
}
#else
#include <hip/hip_runtime_api.h>

static void cpu_checks() {
    float actions[2] = {-7.0f, -7.0f}, logd[2] = {1.0f, 1.0f};
    gymnet_rollout_spec spec{};
    spec.struct_size = sizeof spec; spec.action_source = GYMNET_ACTIONS_ACTOR; spec.steps = 1;
    CHECK(gymnet_vecenv_actor_box_act_logd_device(nullptr, actions, nullptr, logd, 0.0f, 0, 0) == GYMNET_ERR_INVALID_ARG, "act_logd: null handle");
    CHECK(gymnet_vecenv_actor_box_act_logd_device(nullptr, actions, nullptr, nullptr, 0.0f, 0, 0) == GYMNET_ERR_INVALID_ARG, "... also when it forwards");
    CHECK(gymnet_vecenv_rollout_fused_box_logd_device(nullptr, &spec, logd, nullptr) == GYMNET_ERR_INVALID_ARG, "rollout_fused_box_logd: null handle");
    CHECK(gymnet_vecenv_rollout_fused_box_logd_device(nullptr, &spec, nullptr, logd) == GYMNET_ERR_INVALID_ARG, "... with the value pointer alone");
    CHECK(gymnet_vecenv_rollout_fused_box_logd_device(nullptr, &spec, nullptr, nullptr) == GYMNET_ERR_INVALID_ARG, "... also when it forwards");
    CHECK(actions[0] == -7.0f && actions[1] == -7.0f && logd[0] == 1.0f && logd[1] == 1.0f, "nothing written");
    CHECK(GYMNET_ABI_VERSION == 6, "ABI 6");
}

static uint32_t bits(float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; }

static std::vector<float> fetch(const float *d, int64_t count) {
    std::vector<float> out((size_t)count);
    CHECK(hipMemcpy(out.data(), d, sizeof(float) * count, hipMemcpyDeviceToHost) == hipSuccess, "copy");
    return out;
}

static bool all_bits(const std::vector<float> &v, int64_t from, int64_t to, float want) {
    bool all = true;
    for (int64_t k = from; k < to; ++k) all &= bits(v[(size_t)k]) == bits(want);
    return all;
}

static void gpu_checks() {
    const int64_t n = 321, T = 4;
    const float poison = 7.25f;                                  // (a log-density may be positive: sigma < 0.39; none here is 7.25)
    const float c = (float)(-std::log(0.5) - 0.91893853320467274178);
    gymnet::VectorEnv env(GYMNET_ENV_PENDULUM, n, 0, 7, 0);
    env.Reset();
    float *d_act = nullptr, *d_logd = nullptr, *d_rec_act = nullptr, *d_rec_logd = nullptr, *d_rec_value = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_act), sizeof(float) * n) == hipSuccess, "hipMalloc");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_logd), sizeof(float) * n) == hipSuccess, "hipMalloc");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_rec_act), sizeof(float) * T * n) == hipSuccess, "hipMalloc");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_rec_logd), sizeof(float) * (T + 1) * n) == hipSuccess, "hipMalloc");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_rec_value), sizeof(float) * (T + 1) * n) == hipSuccess, "hipMalloc");
    const std::vector<float> fill((size_t)((T + 1) * n), poison);
    CHECK(hipMemcpy(d_rec_logd, fill.data(), sizeof(float) * fill.size(), hipMemcpyHostToDevice) == hipSuccess, "copy");
    CHECK(hipMemcpy(d_rec_value, fill.data(), sizeof(float) * fill.size(), hipMemcpyHostToDevice) == hipSuccess, "copy");
    CHECK(hipMemcpy(d_logd, fill.data(), sizeof(float) * n, hipMemcpyHostToDevice) == hipSuccess, "copy");

    env.ConfigureBoxActor(1, {3, 1}, {0.0f, 0.0f, 0.0f, 0.25f});
    CHECK(gymnet_vecenv_actor_box_act_logd_device(env.handle(), d_act, nullptr, d_logd, 0.0f, 5, 3) == GYMNET_ERR_INVALID_ARG, "a fresh policy has sigma 0");
    CHECK(std::string(gymnet_last_error()).find("sigma") != std::string::npos, "the message names sigma");
    gymnet_rollout_spec spec{};
    spec.struct_size = sizeof spec;
    spec.action_source = GYMNET_ACTIONS_ACTOR; spec.steps = T; spec.epsilon = 0.0f; spec.action_seed = 9; spec.action_tick0 = 100;
    spec.d_rec_actions = d_rec_act;
    CHECK(gymnet_vecenv_rollout_fused_box_logd_device(env.handle(), &spec, d_rec_logd, nullptr) == GYMNET_ERR_INVALID_ARG, "sigma 0: the rollout");
    env.SetBoxActorPolicy(GYMNET_BOX_HEAD_CLAMP, GYMNET_BOX_EXPLORE_GAUSSIAN, 0.5f);
    CHECK(gymnet_vecenv_rollout_fused_box_logd_device(env.handle(), &spec, d_rec_logd, d_rec_value) == GYMNET_ERR_INVALID_ARG, "values without a critic");
    gymnet::check(gymnet_vecenv_sync(env.handle()));
    CHECK(all_bits(fetch(d_logd, n), 0, n, poison) && all_bits(fetch(d_rec_logd, (T + 1) * n), 0, (T + 1) * n, poison), "the refusals wrote nothing");

    env.BoxActorActLogd(d_act, d_logd, 0.0f, 5, 3);
    gymnet::check(gymnet_vecenv_sync(env.handle()));
    CHECK(all_bits(fetch(d_act, n), 0, n, 0.25f), "every lane takes the greedy action");
    CHECK(all_bits(fetch(d_logd, n), 0, n, c), "... whose log-density is c exactly");

    env.ConfigureActorCritic({3, 1}, {0.0f, 0.0f, 0.0f, 2.25f});
    env.RolloutFusedBoxLogd(spec, d_rec_logd, d_rec_value);
    gymnet::check(gymnet_vecenv_sync(env.handle()));
    CHECK(all_bits(fetch(d_rec_act, T * n), 0, T * n, 0.25f), "the fused rollout's actions");
    std::vector<float> rec = fetch(d_rec_logd, (T + 1) * n), val = fetch(d_rec_value, (T + 1) * n);
    CHECK(all_bits(rec, 0, T * n, c) && all_bits(val, 0, T * n, 2.25f), "every step's row holds c and the value");
    CHECK(all_bits(rec, T * n, (T + 1) * n, poison) && all_bits(val, T * n, (T + 1) * n, poison), "the rows after the last step are untouched");
    env.SetBoxActorPolicy(GYMNET_BOX_HEAD_CLAMP, GYMNET_BOX_EXPLORE_SAMPLE, 1.0f);     // c = -ln(2 pi) / 2 from the next launch on
    CHECK(hipMemcpy(d_rec_logd, fill.data(), sizeof(float) * fill.size(), hipMemcpyHostToDevice) == hipSuccess, "copy");
    env.RolloutFusedBoxLogd(spec, nullptr, d_rec_value);
    env.ActorValue(d_rec_value + T * n);
    env.BoxActorActLogd(d_act, d_logd, 0.0f, 5, 3);
    gymnet::check(gymnet_vecenv_sync(env.handle()));
    CHECK(all_bits(fetch(d_rec_value, (T + 1) * n), 0, (T + 1) * n, 2.25f), "values alone, and the last value behind them");
    CHECK(all_bits(fetch(d_rec_logd, (T + 1) * n), 0, (T + 1) * n, poison), "... write no log-density");
    CHECK(all_bits(fetch(d_logd, n), 0, n, (float)(-0.91893853320467274178)), "a new sigma gives a new c");
    env.RolloutFusedBoxLogd(spec, nullptr, nullptr);             // forwards: the plain actor rollout
    env.ConfigureBoxActor(0, {}, {});

    gymnet::VectorEnv discrete(GYMNET_ENV_CARTPOLE, n, 0, 7, 0);
    discrete.Reset();
    discrete.ConfigureActor(1, {4, 2}, {0, 0, 0, 0, 0, 0, 0, 0, 0.5f, 0.5f});
    CHECK(hipMemcpy(d_logd, fill.data(), sizeof(float) * n, hipMemcpyHostToDevice) == hipSuccess, "copy");
    CHECK(gymnet_vecenv_actor_box_act_logd_device(discrete.handle(), d_act, nullptr, d_logd, 0.0f, 5, 3) == GYMNET_ERR_INVALID_ARG, "a Discrete actor");
    CHECK(std::string(gymnet_last_error()).find("gymnet_vecenv_actor_act_logp_device") != std::string::npos, "the message names the Discrete call");
    spec.d_rec_actions = nullptr;
    CHECK(gymnet_vecenv_rollout_fused_box_logd_device(discrete.handle(), &spec, d_rec_logd, nullptr) == GYMNET_ERR_INVALID_ARG, "a Discrete actor's rollout");
    gymnet::check(gymnet_vecenv_sync(discrete.handle()));
    CHECK(all_bits(fetch(d_logd, n), 0, n, poison) && all_bits(fetch(d_rec_logd, (T + 1) * n), 0, (T + 1) * n, poison), "nothing written");
    discrete.ConfigureActor(0, {}, {});
    (void)hipFree(d_act); (void)hipFree(d_logd); (void)hipFree(d_rec_act); (void)hipFree(d_rec_logd); (void)hipFree(d_rec_value);
}
#endif

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
#ifdef LOGD_STUB
    (void)mode;
    stub_checks();
    std::printf("stub: %d failed\n", failed);
#else
    cpu_checks();
    if (mode == "--gpu") gpu_checks();
    std::printf("%s: %d failed\n", mode == "--gpu" ? "cpu+gpu" : "cpu", failed);
#endif
    return failed ? 1 : 0;
}
