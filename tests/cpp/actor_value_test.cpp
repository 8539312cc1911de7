// actor_value_test.cpp — the C++ host side of the critic (gymnet::VectorEnv::ConfigureActorCritic / LoadActorCriticWeights / ActorValue /
// ActorActValue / RolloutFusedValue in include/gymnet_amd.hpp).
//   --stub: built with -DVALUE_STUB against tests/cpp/abi_stub.c and tests/cpp/actor_value_stub.c, under the sanitizers: the five methods
//           hand their arguments across unchanged into buffers of exactly the documented sizes, set struct_size, forward on a null
//           pointer, and throw on a refusal.
//   --cpu:  built against libgymnet_amd.so: the five calls refuse a null handle and write nothing; no GPU needed.
//   --gpu:  a CartPole handle, 321 lanes, a one-layer actor [4, 2] with equal logits and one-layer critics [4, 1] whose value is a
//           constant (zero weights, the bias decides): ActorValue and ActorActValue write it on every lane with ActorActLogp's actions and
//           logp, the fused rollout records it for every step, leaves the row after the last one alone and takes ActorActLogp's actions,
//           LoadActorCriticWeights changes it, and a handle without a critic, a Box actor's rollout and a sampled source are refused.
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

#ifdef VALUE_STUB
extern "C" {
enum { VALUE_STUB_CONFIG = 1, VALUE_STUB_LOAD = 2, VALUE_STUB_VALUE = 3, VALUE_STUB_ACT = 4, VALUE_STUB_ROLLOUT = 5 };
typedef struct value_stub_call {
    int calls, forwarded;
    int log[16];
    int32_t num_layers; int64_t count; float weight_sum;
    float epsilon; uint64_t seed, tick;
    int64_t steps; int32_t action_source;
    const float *value_at;
    int has_critic;
} value_stub_call;
const value_stub_call *value_stub_last(void);
void value_stub_lanes(int64_t n, int32_t input);
}

static void stub_checks() {
    const int64_t n = 37, T = 3;
    gymnet::VectorEnv env(GYMNET_ENV_CARTPOLE, n);
    value_stub_lanes(n, 8);
    const value_stub_call *c = value_stub_last();
    std::vector<float> value((size_t)n, 1.0f);                   // exactly the documented sizes: the sanitizer sees a write past them
    bool refused = false;
    try { env.ActorValue(value.data()); } catch (const std::exception &) { refused = true; }
    CHECK(refused && c->calls == 0 && value[0] == 1.0f, "no critic: a refusal throws and writes nothing");
    // widths {8, 3, 1}: 8 * 3 + 3 + 3 * 1 + 1 = 31 weights, exactly
    std::vector<float> weights(31, 0.5f);
    env.ConfigureActorCritic({8, 3, 1}, weights);
    CHECK(c->calls == 1 && c->log[0] == VALUE_STUB_CONFIG && c->num_layers == 2 && c->count == 31 && c->weight_sum == 15.5f, "widths and weights cross");
    refused = false;
    try { env.ConfigureActorCritic({8, 3, 2}, std::vector<float>(35, 0.0f)); } catch (const std::exception &) { refused = true; }
    CHECK(refused && c->calls == 1 && c->has_critic == 1, "a last width other than 1 throws, the critic stays");
    std::fill(weights.begin(), weights.end(), 0.25f);
    env.LoadActorCriticWeights(weights.data(), (int64_t)weights.size());
    CHECK(c->calls == 2 && c->log[1] == VALUE_STUB_LOAD && c->weight_sum == 7.75f, "the new weights cross");
    env.ActorValue(value.data());
    CHECK(c->calls == 3 && c->log[2] == VALUE_STUB_VALUE && c->value_at == value.data() && value[n - 1] == 1000.0f + (float)(n - 1), "the value pointer crosses");

    std::vector<int32_t> actions((size_t)n, -7);
    std::vector<float> logp((size_t)n, 1.0f), logits((size_t)n * 2, -7.0f);
    std::fill(value.begin(), value.end(), 1.0f);
    env.ActorActValue(actions.data(), logp.data(), value.data(), 0.25f, 5, 3);
    CHECK(c->calls == 4 && c->log[3] == VALUE_STUB_ACT && c->forwarded == 0 && c->epsilon == 0.25f && c->seed == 5 && c->tick == 3, "arguments cross unchanged");
    CHECK(actions[n - 1] == (int32_t)((n - 1) & 1) && logp[n - 1] == -(float)(n - 1) && value[n - 1] == 1000.0f + (float)(n - 1) && logits[0] == -7.0f,
          "actions, logp and value written, no logits");
    std::fill(logp.begin(), logp.end(), 1.0f);
    env.ActorActValue(actions.data(), nullptr, value.data(), 1.0f, 6, 4, logits.data());
    CHECK(c->calls == 5 && logits[2 * n - 1] == 1.0f && logp[n - 1] == 1.0f, "the logits pointer crosses, a null logp stays null");
    env.ActorActValue(actions.data(), logp.data(), value.data());
    CHECK(c->calls == 6 && c->epsilon == 0.0f && c->seed == 0 && c->tick == 0, "the defaults are ActorAct's");
    std::fill(value.begin(), value.end(), 1.0f);
    env.ActorActValue(actions.data(), logp.data(), nullptr, 0.5f, 1, 2);
    CHECK(c->calls == 7 && c->forwarded == 1 && value[0] == 1.0f, "a null value forwards");
    refused = false;
    try { env.ActorActValue(actions.data(), logp.data(), value.data(), 1.5f); } catch (const std::exception &) { refused = true; }
    CHECK(refused && c->calls == 7, "a refusal throws");

    std::vector<float> rec((size_t)(T * n), 1.0f), rec_logp((size_t)(T * n), 1.0f);
    std::vector<int32_t> rec_act((size_t)(T * n), -7);
    gymnet_rollout_spec spec{};
    spec.action_source = GYMNET_ACTIONS_ACTOR; spec.steps = T; spec.epsilon = 0.75f; spec.action_seed = 9; spec.action_tick0 = 100;
    spec.d_rec_actions = rec_act.data();
    env.RolloutFusedValue(spec, rec_logp.data(), rec.data());    // (struct_size is the wrapper's to set: the stub refuses any other)
    CHECK(c->calls == 8 && c->log[7] == VALUE_STUB_ROLLOUT && c->forwarded == 1 && c->steps == T && c->action_source == GYMNET_ACTIONS_ACTOR, "the spec crosses");
    CHECK(c->epsilon == 0.75f && c->seed == 9 && c->tick == 100, "... with its action stream");
    CHECK(rec[(size_t)(T * n - 1)] == (float)(T * n - 1) && rec_logp[(size_t)(T * n - 1)] == -(float)(T * n - 1) &&
          rec_act[(size_t)(T * n - 1)] == (int32_t)((T * n - 1) & 1), "every row written");
    std::fill(rec_logp.begin(), rec_logp.end(), 1.0f);
    env.RolloutFusedValue(spec, nullptr, rec.data());
    CHECK(c->calls == 9 && c->forwarded == 1 && rec_logp[0] == 1.0f, "d_rec_logp may be null");
    std::fill(rec.begin(), rec.end(), 1.0f);
    env.RolloutFusedValue(spec, rec_logp.data(), nullptr);
    CHECK(c->calls == 10 && c->forwarded == 2 && rec[0] == 1.0f && rec_logp[1] == -1.0f, "a null d_rec_value forwards");
    spec.action_source = GYMNET_ACTIONS_SAMPLE;
    refused = false;
    try { env.RolloutFusedValue(spec, nullptr, rec.data()); } catch (const std::exception &) { refused = true; }
    CHECK(refused && c->calls == 10 && rec[0] == 1.0f, "a source other than the actor throws and writes nothing");
    env.ConfigureActorCritic({}, {});
    CHECK(c->calls == 11 && c->log[10] == VALUE_STUB_CONFIG && c->num_layers == 0 && c->has_critic == 0, "empty widths remove the critic");
    refused = false;
    try { env.ActorValue(value.data()); } catch (const std::exception &) { refused = true; }
    CHECK(refused && c->calls == 11, "... and a value is refused after it");
}
#else
#include <hip/hip_runtime_api.h>

static void cpu_checks() {
    int32_t actions[2] = {-7, -7}, widths[2] = {4, 1};
    float value[2] = {1.0f, 1.0f}, weights[5] = {0, 0, 0, 0, 0};
    gymnet_rollout_spec spec{};
    spec.struct_size = sizeof spec; spec.action_source = GYMNET_ACTIONS_ACTOR; spec.steps = 1;
    CHECK(gymnet_vecenv_actor_critic_config(nullptr, 1, widths, weights, 5) == GYMNET_ERR_INVALID_ARG, "critic_config: null handle");
    CHECK(gymnet_vecenv_actor_critic_load_device(nullptr, weights, 5) == GYMNET_ERR_INVALID_ARG, "critic_load: null handle");
    CHECK(gymnet_vecenv_actor_value_device(nullptr, value) == GYMNET_ERR_INVALID_ARG, "value: null handle");
    CHECK(gymnet_vecenv_actor_act_value_device(nullptr, actions, nullptr, nullptr, value, 0.0f, 0, 0) == GYMNET_ERR_INVALID_ARG, "act_value: null handle");
    CHECK(gymnet_vecenv_actor_act_value_device(nullptr, actions, nullptr, nullptr, nullptr, 0.0f, 0, 0) == GYMNET_ERR_INVALID_ARG, "... also when it forwards");
    CHECK(gymnet_vecenv_rollout_fused_value_device(nullptr, &spec, nullptr, value) == GYMNET_ERR_INVALID_ARG, "rollout_fused_value: null handle");
    CHECK(gymnet_vecenv_rollout_fused_value_device(nullptr, &spec, nullptr, nullptr) == GYMNET_ERR_INVALID_ARG, "... also when it forwards");
    CHECK(actions[0] == -7 && actions[1] == -7 && value[0] == 1.0f && value[1] == 1.0f, "nothing written");
    CHECK(GYMNET_ABI_VERSION == 6, "ABI 6");
}

static uint32_t bits(float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; }

template <class T>
static std::vector<T> fetch(const T *d, int64_t count) {
    std::vector<T> out((size_t)count);
    CHECK(hipMemcpy(out.data(), d, sizeof(T) * count, hipMemcpyDeviceToHost) == hipSuccess, "copy");
    return out;
}

static bool all_bits(const std::vector<float> &v, int64_t from, int64_t to, float want) {
    bool all = true;
    for (int64_t k = from; k < to; ++k) all &= bits(v[(size_t)k]) == bits(want);
    return all;
}

static void gpu_checks() {
    const int64_t n = 321, T = 4;
    const float poison = -7.25f;
    gymnet::VectorEnv env(GYMNET_ENV_CARTPOLE, n, 0, 7, 0);
    env.Reset();
    const std::vector<float> equal = {0, 0, 0, 0, 0, 0, 0, 0, 0.5f, 0.5f};           // the actor: W = 0, b = (0.5, 0.5)
    const std::vector<float> flat = {0, 0, 0, 0, 0.625f}, other = {0, 0, 0, 0, -1.5f};    // the critics: W = 0, b = the value
    int32_t *d_act = nullptr, *d_rec_act = nullptr;
    float *d_logp = nullptr, *d_value = nullptr, *d_rec = nullptr, *d_rec_logp = nullptr, *d_w = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_act), sizeof(int32_t) * n) == hipSuccess, "hipMalloc");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_rec_act), sizeof(int32_t) * T * n) == hipSuccess, "hipMalloc");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_logp), sizeof(float) * n) == hipSuccess, "hipMalloc");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_value), sizeof(float) * n) == hipSuccess, "hipMalloc");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_rec), sizeof(float) * (T + 1) * n) == hipSuccess, "hipMalloc");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_rec_logp), sizeof(float) * T * n) == hipSuccess, "hipMalloc");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_w), sizeof(float) * other.size()) == hipSuccess, "hipMalloc");
    const std::vector<float> fill((size_t)((T + 1) * n), poison);
    CHECK(hipMemcpy(d_rec, fill.data(), sizeof(float) * fill.size(), hipMemcpyHostToDevice) == hipSuccess, "copy");
    CHECK(hipMemcpy(d_value, fill.data(), sizeof(float) * n, hipMemcpyHostToDevice) == hipSuccess, "copy");

    CHECK(gymnet_vecenv_actor_critic_config(env.handle(), 1, std::vector<int32_t>{4, 1}.data(), flat.data(), 5) == GYMNET_ERR_INVALID_ARG, "a critic needs an actor");
    env.ConfigureActor(1, {4, 2}, equal);
    CHECK(gymnet_vecenv_actor_value_device(env.handle(), d_value) == GYMNET_ERR_INVALID_ARG, "no critic");
    gymnet_rollout_spec spec{};
    spec.struct_size = sizeof spec;
    spec.action_source = GYMNET_ACTIONS_ACTOR; spec.steps = T; spec.epsilon = 1.0f; spec.action_seed = 9; spec.action_tick0 = 100;
    spec.d_rec_actions = d_rec_act;
    CHECK(gymnet_vecenv_rollout_fused_value_device(env.handle(), &spec, nullptr, d_rec) == GYMNET_ERR_INVALID_ARG, "no critic: the rollout");
    CHECK(gymnet_vecenv_actor_critic_config(env.handle(), 1, std::vector<int32_t>{4, 2}.data(), equal.data(), 10) == GYMNET_ERR_INVALID_ARG, "a last width of 2");
    env.ConfigureActorCritic({4, 1}, flat);
    env.ActorValue(d_value);
    gymnet::check(gymnet_vecenv_sync(env.handle()));
    CHECK(all_bits(fetch(d_value, n), 0, n, 0.625f), "the bias on every lane");

    env.ActorActLogp(d_act, d_logp, 1.0f, 5, 3);
    gymnet::check(gymnet_vecenv_sync(env.handle()));
    const std::vector<int32_t> plain = fetch(d_act, n);
    const std::vector<float> plain_logp = fetch(d_logp, n);
    CHECK(hipMemcpy(d_value, fill.data(), sizeof(float) * n, hipMemcpyHostToDevice) == hipSuccess, "copy");
    env.ActorActValue(d_act, d_logp, d_value, 1.0f, 5, 3);
    gymnet::check(gymnet_vecenv_sync(env.handle()));
    CHECK(fetch(d_act, n) == plain && std::memcmp(fetch(d_logp, n).data(), plain_logp.data(), sizeof(float) * n) == 0, "actions and logp are ActorActLogp's");
    CHECK(all_bits(fetch(d_value, n), 0, n, 0.625f), "... with the value beside them");

    // the fused rollout against steps x (ActorActLogp, StepDevice, PushActor) on a second handle
    gymnet::VectorEnv loop(GYMNET_ENV_CARTPOLE, n, 0, 7, 0);
    loop.Reset();
    loop.ConfigureActor(1, {4, 2}, equal);
    std::vector<int32_t> want_act;
    for (int64_t t = 0; t < T; ++t) {
        loop.ActorActLogp(d_act, d_logp, 1.0f, 9, 100 + (uint64_t)t);
        loop.StepDevice(d_act);
        loop.PushActor();
        gymnet::check(gymnet_vecenv_sync(loop.handle()));
        const std::vector<int32_t> a = fetch(d_act, n);
        want_act.insert(want_act.end(), a.begin(), a.end());
    }
    env.RolloutFusedValue(spec, d_rec_logp, d_rec);
    gymnet::check(gymnet_vecenv_sync(env.handle()));
    CHECK(fetch(d_rec_act, T * n) == want_act, "the fused rollout's actions are the loop's");
    std::vector<float> rec = fetch(d_rec, (T + 1) * n);
    CHECK(all_bits(rec, 0, T * n, 0.625f), "every step's row holds the value");
    CHECK(all_bits(rec, T * n, (T + 1) * n, poison), "the row after the last step is untouched");
    CHECK(all_bits(fetch(d_rec_logp, T * n), 0, T * n, plain_logp[0]), "... and logp is recorded beside it");

    CHECK(hipMemcpy(d_w, other.data(), sizeof(float) * other.size(), hipMemcpyHostToDevice) == hipSuccess, "copy");
    env.LoadActorCriticWeights(d_w, (int64_t)other.size());
    env.RolloutFusedValue(spec, nullptr, d_rec);
    env.ActorValue(d_rec + T * n);
    gymnet::check(gymnet_vecenv_sync(env.handle()));
    rec = fetch(d_rec, (T + 1) * n);
    CHECK(all_bits(rec, 0, (T + 1) * n, -1.5f), "new weights: every row, and the last value behind them");
    spec.action_source = GYMNET_ACTIONS_SAMPLE;
    bool refused = false;
    try { env.RolloutFusedValue(spec, nullptr, d_rec); } catch (const std::exception &) { refused = true; }
    CHECK(refused, "a source other than the actor is refused");
    spec.action_source = GYMNET_ACTIONS_ACTOR;
    env.RolloutFusedValue(spec, nullptr, nullptr);                // forwards: the plain actor rollout
    env.ConfigureActorCritic({}, {});
    CHECK(gymnet_vecenv_actor_value_device(env.handle(), d_value) == GYMNET_ERR_INVALID_ARG, "removed: no value");
    env.ConfigureActor(0, {}, {});
    loop.ConfigureActor(0, {}, {});

    gymnet::VectorEnv box(GYMNET_ENV_PENDULUM, n, 0, 7, 0);      // a Box actor: the stand-alone value serves it, the fused rollout does not
    box.Reset();
    box.ConfigureBoxActor(1, {3, 1}, {0.0f, 0.0f, 1.0f, 0.0f});
    box.ConfigureActorCritic({3, 1}, {0.0f, 0.0f, 0.0f, 2.25f});
    box.ActorValue(d_value);
    gymnet::check(gymnet_vecenv_sync(box.handle()));
    CHECK(all_bits(fetch(d_value, n), 0, n, 2.25f), "a Box actor's value");
    CHECK(hipMemcpy(d_rec, fill.data(), sizeof(float) * fill.size(), hipMemcpyHostToDevice) == hipSuccess, "copy");
    spec.struct_size = sizeof spec;
    CHECK(gymnet_vecenv_rollout_fused_value_device(box.handle(), &spec, nullptr, d_rec) == GYMNET_ERR_INVALID_ARG, "a Box actor's rollout");
    CHECK(std::string(gymnet_last_error()).find("Box") != std::string::npos, "the message names Box");
    gymnet::check(gymnet_vecenv_sync(box.handle()));
    CHECK(all_bits(fetch(d_rec, (T + 1) * n), 0, (T + 1) * n, poison), "nothing written");
    box.ConfigureBoxActor(0, {}, {});
    (void)hipFree(d_act); (void)hipFree(d_rec_act); (void)hipFree(d_logp); (void)hipFree(d_value); (void)hipFree(d_rec); (void)hipFree(d_rec_logp); (void)hipFree(d_w);
}
#endif

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
#ifdef VALUE_STUB
    stub_checks();
    std::printf("stub: %d failed\n", failed);
#else
    cpu_checks();
    if (mode == "--gpu") gpu_checks();
    std::printf("%s: %d failed\n", mode == "--gpu" ? "cpu+gpu" : "cpu", failed);
#endif
    return failed ? 1 : 0;
}
