// actor_logp_test.cpp — the C++ host side of the log-probability a Discrete actor records (gymnet::VectorEnv::ActorActLogp /
// RolloutFusedLogp in include/gymnet_amd.hpp).
//   --stub: built with -DLOGP_STUB against tests/cpp/abi_stub.c and tests/cpp/actor_logp_stub.c, under the sanitizers: the two methods
//           hand their arguments across unchanged into buffers of exactly the documented sizes, set struct_size, forward on a null
//           pointer, and throw on a refusal.
//   --cpu:  built against libgymnet_amd.so: the two calls refuse a null handle; on a machine without a GPU the handle they would belong
//           to is refused with NO_DEVICE; no GPU needed.
//   --gpu:  a CartPole handle, 321 lanes, one-layer nets [4, 2] whose logits are constants (zero weights, the biases decide).  Equal
//           logits: logp is -log_pos(2) on every lane whatever it takes, with actions equal to ActorAct's.  A logit gap of 1000 at
//           temperature 1: +0 on the lanes that take the greedy action, exactly -1000 on the others (uniform exploration at epsilon 1).
//           The fused rollout records the same values for every step, leaves the row after the last one alone, and equals steps x
//           (ActorActLogp, StepDevice, PushActor) in its recorded actions.  A Box actor and a ring source are refused.
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

#ifdef LOGP_STUB
extern "C" {
typedef struct logp_stub_call {
    int acts, rollouts, forwarded;
    float epsilon; uint64_t seed, tick;
    int64_t steps; int32_t action_source;
} logp_stub_call;
const logp_stub_call *logp_stub_last(void);
void logp_stub_lanes(int64_t n);
}

static void stub_checks() {
    const int64_t n = 37, T = 3;
    gymnet::VectorEnv env(GYMNET_ENV_CARTPOLE, n);
    logp_stub_lanes(n);
    const logp_stub_call *c = logp_stub_last();
    std::vector<int32_t> actions((size_t)n, -7);                 // exactly the documented sizes: the sanitizer sees a write past them
    std::vector<float> logp((size_t)n, 1.0f), logits((size_t)n * 2, -7.0f);
    env.ActorActLogp(actions.data(), logp.data(), 0.25f, 5, 3);
    CHECK(c->acts == 1 && c->forwarded == 0 && c->epsilon == 0.25f && c->seed == 5 && c->tick == 3, "arguments cross unchanged");
    CHECK(actions[n - 1] == (int32_t)((n - 1) & 1) && logp[n - 1] == -(float)(n - 1) && logits[0] == -7.0f, "actions and logp written, no logits");
    env.ActorActLogp(actions.data(), logp.data(), 1.0f, 6, 4, logits.data());
    CHECK(c->acts == 2 && logits[2 * n - 1] == 1.0f, "the logits pointer crosses");
    env.ActorActLogp(actions.data(), logp.data());
    CHECK(c->acts == 3 && c->epsilon == 0.0f && c->seed == 0 && c->tick == 0, "the defaults are ActorAct's");
    std::fill(logp.begin(), logp.end(), 1.0f);
    env.ActorActLogp(actions.data(), nullptr, 0.5f, 1, 2);
    CHECK(c->acts == 4 && c->forwarded == 1 && logp[0] == 1.0f, "a null logp forwards");
    bool refused = false;
    try { env.ActorActLogp(actions.data(), logp.data(), 1.5f); } catch (const std::exception &) { refused = true; }
    CHECK(refused && c->acts == 4, "a refusal throws");

    std::vector<float> rec((size_t)(T * n), 1.0f);
    std::vector<int32_t> rec_act((size_t)(T * n), -7);
    gymnet_rollout_spec spec{};
    spec.action_source = GYMNET_ACTIONS_ACTOR; spec.steps = T; spec.epsilon = 0.75f; spec.action_seed = 9; spec.action_tick0 = 100;
    spec.d_rec_actions = rec_act.data();
    env.RolloutFusedLogp(spec, rec.data());                      // (struct_size is the wrapper's to set: the stub refuses any other)
    CHECK(c->rollouts == 1 && c->forwarded == 1 && c->steps == T && c->action_source == GYMNET_ACTIONS_ACTOR, "the spec crosses");
    CHECK(c->epsilon == 0.75f && c->seed == 9 && c->tick == 100, "... with its action stream");
    CHECK(rec[(size_t)(T * n - 1)] == -(float)(T * n - 1) && rec_act[(size_t)(T * n - 1)] == (int32_t)((T * n - 1) & 1), "every row written");
    std::fill(rec.begin(), rec.end(), 1.0f);
    env.RolloutFusedLogp(spec, nullptr);
    CHECK(c->rollouts == 2 && c->forwarded == 2 && rec[0] == 1.0f, "a null d_rec_logp forwards");
    spec.action_source = GYMNET_ACTIONS_SAMPLE;
    refused = false;
    try { env.RolloutFusedLogp(spec, rec.data()); } catch (const std::exception &) { refused = true; }
    CHECK(refused && c->rollouts == 2 && rec[0] == 1.0f, "a source other than the actor throws and writes nothing");
}
#else
#include <hip/hip_runtime_api.h>

static void cpu_checks(bool gpu) {
    int32_t actions[2] = {-7, -7};
    float logp[2] = {1.0f, 1.0f};
    gymnet_rollout_spec spec{};
    spec.struct_size = sizeof spec; spec.action_source = GYMNET_ACTIONS_ACTOR; spec.steps = 1;
    CHECK(gymnet_vecenv_actor_act_logp_device(nullptr, actions, nullptr, logp, 0.0f, 0, 0) == GYMNET_ERR_INVALID_ARG, "act_logp: null handle");
    CHECK(gymnet_vecenv_actor_act_logp_device(nullptr, actions, nullptr, nullptr, 0.0f, 0, 0) == GYMNET_ERR_INVALID_ARG, "... also when it forwards");
    CHECK(gymnet_vecenv_rollout_fused_logp_device(nullptr, &spec, logp) == GYMNET_ERR_INVALID_ARG, "rollout_fused_logp: null handle");
    CHECK(gymnet_vecenv_rollout_fused_logp_device(nullptr, &spec, nullptr) == GYMNET_ERR_INVALID_ARG, "... also when it forwards");
    CHECK(actions[0] == -7 && actions[1] == -7 && logp[0] == 1.0f && logp[1] == 1.0f, "nothing written");
    CHECK(GYMNET_ABI_VERSION == 6, "ABI 6");
    int ndev = 0;
    if (!gpu && gymnet_device_count(&ndev) != GYMNET_OK) {
        // no GPU here: the engine refuses loudly, a log-probability never comes from a CPU path
        CHECK(ndev == 0, "count reported as 0");
        bool no_device = false;
        try { gymnet::VectorEnv e(GYMNET_ENV_CARTPOLE, 16); } catch (const gymnet::NoDeviceError &) { no_device = true; }
        CHECK(no_device, "no device -> NoDeviceError");
    }
}

static uint32_t bits(float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; }

template <class T>
static std::vector<T> fetch(const T *d, int64_t count) {
    std::vector<T> out((size_t)count);
    CHECK(hipMemcpy(out.data(), d, sizeof(T) * count, hipMemcpyDeviceToHost) == hipSuccess, "copy");
    return out;
}

static void gpu_checks() {
    const int64_t n = 321, T = 4;
    const float poison = -7.25f;
    gymnet::VectorEnv env(GYMNET_ENV_CARTPOLE, n, 0, 7, 0);
    env.Reset();
    const std::vector<float> equal = {0, 0, 0, 0, 0, 0, 0, 0, 0.5f, 0.5f};           // W = 0, b = (0.5, 0.5)
    const std::vector<float> apart = {0, 0, 0, 0, 0, 0, 0, 0, 0.0f, 1000.0f};        // b = (0, 1000): action 1, by far
    int32_t *d_act = nullptr, *d_rec_act = nullptr;
    float *d_logp = nullptr, *d_rec = nullptr, *d_w = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_act), sizeof(int32_t) * n) == hipSuccess, "hipMalloc");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_rec_act), sizeof(int32_t) * T * n) == hipSuccess, "hipMalloc");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_logp), sizeof(float) * n) == hipSuccess, "hipMalloc");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_rec), sizeof(float) * (T + 1) * n) == hipSuccess, "hipMalloc");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_w), sizeof(float) * apart.size()) == hipSuccess, "hipMalloc");
    const std::vector<float> fill((size_t)((T + 1) * n), poison);
    CHECK(hipMemcpy(d_rec, fill.data(), sizeof(float) * fill.size(), hipMemcpyHostToDevice) == hipSuccess, "copy");
    CHECK(hipMemcpy(d_logp, fill.data(), sizeof(float) * n, hipMemcpyHostToDevice) == hipSuccess, "copy");

    CHECK(gymnet_vecenv_actor_act_logp_device(env.handle(), d_act, nullptr, d_logp, 0.5f, 5, 3) == GYMNET_ERR_INVALID_ARG, "no actor");
    env.ConfigureActor(1, {4, 2}, equal);
    // equal logits: S = 2, logp = a_j - log_pos(2) = 0 - (0.693359375f + -2.12194440e-4f) whatever the lane takes
    const float ln2 = 0.693359375f + -2.12194440e-4f;
    CHECK(std::fabs((double)ln2 - std::log(2.0)) < 1.2e-7, "log_pos(2)");
    env.ActorAct(d_act, 1.0f, 5, 3);
    gymnet::check(gymnet_vecenv_sync(env.handle()));
    const std::vector<int32_t> plain = fetch(d_act, n);
    env.ActorActLogp(d_act, d_logp, 1.0f, 5, 3);
    gymnet::check(gymnet_vecenv_sync(env.handle()));
    CHECK(fetch(d_act, n) == plain, "the actions are ActorAct's");
    int ones = 0;
    bool all = true;
    for (int32_t a : plain) ones += a == 1;
    for (float v : fetch(d_logp, n)) all &= bits(v) == bits(-ln2);
    CHECK(ones > n / 4 && ones < 3 * n / 4, "both actions occur");
    CHECK(all, "equal logits: -log_pos(2) on every lane");

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
    gymnet_rollout_spec spec{};
    spec.action_source = GYMNET_ACTIONS_ACTOR; spec.steps = T; spec.epsilon = 1.0f; spec.action_seed = 9; spec.action_tick0 = 100;
    spec.d_rec_actions = d_rec_act;
    env.RolloutFusedLogp(spec, d_rec);
    gymnet::check(gymnet_vecenv_sync(env.handle()));
    CHECK(fetch(d_rec_act, T * n) == want_act, "the fused rollout's actions are the loop's");
    const std::vector<float> rec = fetch(d_rec, (T + 1) * n);
    all = true;
    for (int64_t k = 0; k < T * n; ++k) all &= bits(rec[(size_t)k]) == bits(-ln2);
    CHECK(all, "every step's row holds -log_pos(2)");
    all = true;
    for (int64_t k = T * n; k < (T + 1) * n; ++k) all &= rec[(size_t)k] == poison;
    CHECK(all, "the row after the last step is untouched");
    spec.action_source = GYMNET_ACTIONS_SAMPLE;
    bool refused = false;
    try { env.RolloutFusedLogp(spec, d_rec); } catch (const std::exception &) { refused = true; }
    CHECK(refused, "a source other than the actor is refused");
    spec.action_source = GYMNET_ACTIONS_ACTOR;
    env.RolloutFusedLogp(spec, nullptr);                          // forwards: the plain actor rollout

    // a gap of 1000 at temperature 1 under uniform exploration: +0 where the lane takes action 1, -1000 where it takes action 0
    CHECK(hipMemcpy(d_w, apart.data(), sizeof(float) * apart.size(), hipMemcpyHostToDevice) == hipSuccess, "copy");
    env.LoadActorWeights(d_w, (int64_t)apart.size());
    env.ActorActLogp(d_act, d_logp, 1.0f, 5, 3);
    gymnet::check(gymnet_vecenv_sync(env.handle()));
    const std::vector<int32_t> taken = fetch(d_act, n);
    const std::vector<float> lp = fetch(d_logp, n);
    all = true;
    ones = 0;
    for (int64_t i = 0; i < n; ++i) {
        ones += taken[(size_t)i] == 1;
        all &= bits(lp[(size_t)i]) == (taken[(size_t)i] == 1 ? bits(0.0f) : bits(-1000.0f));
    }
    CHECK(all && ones > n / 4 && ones < 3 * n / 4, "a gap of 1000: +0 for the greedy action, -1000 for the other");
    env.SetActorExploration(GYMNET_ACTOR_EXPLORE_SOFTMAX, 1.0f);
    env.ActorActLogp(d_act, d_logp, 1.0f, 5, 3);
    gymnet::check(gymnet_vecenv_sync(env.handle()));
    all = true;
    for (int32_t a : fetch(d_act, n)) all &= a == 1;
    for (float v : fetch(d_logp, n)) all &= bits(v) == bits(0.0f);
    CHECK(all, "... and under softmax every lane takes the greedy action at logp +0");
    env.ConfigureActor(0, {}, {});
    loop.ConfigureActor(0, {}, {});

    gymnet::VectorEnv box(GYMNET_ENV_PENDULUM, n, 0, 7, 0);      // a Box actor is refused, and the message says so
    box.Reset();
    box.ConfigureBoxActor(1, {3, 1}, {0.0f, 0.0f, 1.0f, 0.0f});
    CHECK(hipMemcpy(d_logp, fill.data(), sizeof(float) * n, hipMemcpyHostToDevice) == hipSuccess, "copy");
    CHECK(gymnet_vecenv_actor_act_logp_device(box.handle(), d_act, nullptr, d_logp, 0.5f, 5, 3) == GYMNET_ERR_INVALID_ARG, "a Box actor");
    CHECK(std::string(gymnet_last_error()).find("Box") != std::string::npos, "the message names Box");
    spec.struct_size = sizeof spec;
    CHECK(gymnet_vecenv_rollout_fused_logp_device(box.handle(), &spec, d_rec) == GYMNET_ERR_INVALID_ARG, "a Box actor's rollout");
    CHECK(std::string(gymnet_last_error()).find("Box") != std::string::npos, "the message names Box");
    gymnet::check(gymnet_vecenv_sync(box.handle()));
    all = true;
    for (float v : fetch(d_logp, n)) all &= v == poison;
    CHECK(all, "nothing written");
    box.ConfigureBoxActor(0, {}, {});
    (void)hipFree(d_act); (void)hipFree(d_rec_act); (void)hipFree(d_logp); (void)hipFree(d_rec); (void)hipFree(d_w);
}
#endif

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
#ifdef LOGP_STUB
    stub_checks();
    std::printf("stub: %d failed\n", failed);
#else
    cpu_checks(mode == "--gpu");
    if (mode == "--gpu") gpu_checks();
    std::printf("%s: %d failed\n", mode == "--gpu" ? "cpu+gpu" : "cpu", failed);
#endif
    return failed ? 1 : 0;
}
