// actor_softmax_test.cpp — the C++ host side of a Discrete actor's exploration setting (gymnet::VectorEnv::SetActorExploration /
// GetActorExploration in include/gymnet_amd.hpp).
//   --stub: built with -DSOFTMAX_STUB against tests/cpp/abi_stub.c and tests/cpp/actor_softmax_stub.c, under the sanitizers: the two
//           methods hand their arguments across unchanged, the default temperature is 1, a refusal throws and changes nothing.
//   --cpu:  built against libgymnet_amd.so: the two calls refuse a null handle and write nothing; on a machine without a GPU the handle a
//           setting would belong to is refused with NO_DEVICE; no GPU needed.
//   --gpu:  a CartPole handle, 321 lanes, one-layer nets [4, 2] whose logits are constants (zero weights, the biases decide).  Equal logits:
//           under SOFTMAX at epsilon 1 the action is floor(2 u) — the top bit of word A, which is also what UNIFORM draws, so the two
//           settings agree bit for bit and both actions occur.  A logit gap of 1000 (> 104 * temperature): every lane takes the greedy
//           action under SOFTMAX at epsilon 1 while UNIFORM leaves it on about half.  The setting round-trips, bad arguments are refused
//           and leave it, push / load keep it, a re-config returns it to the default.
#include <cmath>
#include <cstdint>
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

#ifdef SOFTMAX_STUB
extern "C" {
typedef struct softmax_stub_call { int sets, gets; int32_t explore; float temperature; } softmax_stub_call;
const softmax_stub_call *softmax_stub_last(void);
}

static void stub_checks() {
    gymnet::VectorEnv env(GYMNET_ENV_CARTPOLE, 37);
    const softmax_stub_call *c = softmax_stub_last();
    gymnet_actor_explore explore = GYMNET_ACTOR_EXPLORE_SOFTMAX;
    float temperature = -1.0f;
    env.GetActorExploration(explore, temperature);
    CHECK(c->gets == 1 && explore == GYMNET_ACTOR_EXPLORE_UNIFORM && temperature == 1.0f, "the default");
    env.SetActorExploration(GYMNET_ACTOR_EXPLORE_SOFTMAX, 0.25f);
    CHECK(c->sets == 1 && c->explore == GYMNET_ACTOR_EXPLORE_SOFTMAX && c->temperature == 0.25f, "arguments cross unchanged");
    env.SetActorExploration(GYMNET_ACTOR_EXPLORE_SOFTMAX);
    CHECK(c->sets == 2 && c->temperature == 1.0f, "the default temperature is 1");
    env.SetActorExploration(GYMNET_ACTOR_EXPLORE_SOFTMAX, 4.0f);
    const float bad[5] = {std::numeric_limits<float>::quiet_NaN(), 0.0f, -1.0f, std::numeric_limits<float>::infinity(), 1e-39f};
    for (float t : bad) {
        bool refused = false;
        try { env.SetActorExploration(GYMNET_ACTOR_EXPLORE_SOFTMAX, t); } catch (const std::exception &) { refused = true; }
        CHECK(refused && c->sets == 3, "a bad temperature throws");
    }
    bool refused = false;
    try { env.SetActorExploration((gymnet_actor_explore)2, 1.0f); } catch (const std::exception &) { refused = true; }
    CHECK(refused && c->sets == 3, "an unknown enum value throws");
    env.GetActorExploration(explore, temperature);
    CHECK(explore == GYMNET_ACTOR_EXPLORE_SOFTMAX && temperature == 4.0f, "refusals leave the setting; it round-trips");
    CHECK(gymnet_vecenv_actor_get_exploration(env.handle(), nullptr, nullptr) == GYMNET_OK, "any out pointer may be null");
}
#else
#include <hip/hip_runtime_api.h>

static void cpu_checks(bool gpu) {
    int32_t explore = -9;
    float temperature = -9.0f;
    CHECK(gymnet_vecenv_actor_set_exploration(nullptr, GYMNET_ACTOR_EXPLORE_SOFTMAX, 1.0f) == GYMNET_ERR_INVALID_ARG, "set_exploration");
    CHECK(gymnet_vecenv_actor_get_exploration(nullptr, &explore, &temperature) == GYMNET_ERR_INVALID_ARG, "get_exploration");
    CHECK(explore == -9 && temperature == -9.0f, "nothing written");
    CHECK(GYMNET_ACTOR_EXPLORE_UNIFORM == 0 && GYMNET_ACTOR_EXPLORE_SOFTMAX == 1, "enum values");
    CHECK(GYMNET_ABI_VERSION == 6, "ABI 6");
    int ndev = 0;
    if (!gpu && gymnet_device_count(&ndev) != GYMNET_OK) {
        // no GPU here: the engine refuses loudly, a setting never reaches a CPU path
        CHECK(ndev == 0, "count reported as 0");
        bool no_device = false;
        try { gymnet::VectorEnv e(GYMNET_ENV_CARTPOLE, 16); } catch (const gymnet::NoDeviceError &) { no_device = true; }
        CHECK(no_device, "no device -> NoDeviceError");
    }
}

static std::vector<int32_t> act(gymnet::VectorEnv &env, int32_t *d_act, float epsilon, int64_t n) {
    env.ActorAct(d_act, epsilon, 5, 3);
    gymnet::check(gymnet_vecenv_sync(env.handle()));
    std::vector<int32_t> out((size_t)n);
    CHECK(hipMemcpy(out.data(), d_act, sizeof(int32_t) * n, hipMemcpyDeviceToHost) == hipSuccess, "copy");
    return out;
}

static void gpu_checks() {
    const int64_t n = 321;
    gymnet::VectorEnv env(GYMNET_ENV_CARTPOLE, n, 0, 7, 0);
    env.Reset();
    const std::vector<float> equal = {0, 0, 0, 0, 0, 0, 0, 0, 0.5f, 0.5f};           // W = 0, b = (0.5, 0.5)
    const std::vector<float> apart = {0, 0, 0, 0, 0, 0, 0, 0, 0.0f, 1000.0f};        // b = (0, 1000): action 1, by far
    CHECK(gymnet_vecenv_actor_set_exploration(env.handle(), GYMNET_ACTOR_EXPLORE_SOFTMAX, 1.0f) == GYMNET_ERR_INVALID_ARG, "no actor");
    env.ConfigureActor(1, {4, 2}, equal);
    gymnet_actor_explore explore = GYMNET_ACTOR_EXPLORE_SOFTMAX;
    float temperature = -1.0f;
    env.GetActorExploration(explore, temperature);
    CHECK(explore == GYMNET_ACTOR_EXPLORE_UNIFORM && temperature == 1.0f, "a new actor has the default setting");
    int32_t *d_act = nullptr;
    float *d_w = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_act), sizeof(int32_t) * n) == hipSuccess, "hipMalloc");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_w), sizeof(float) * apart.size()) == hipSuccess, "hipMalloc");

    const std::vector<int32_t> uniform = act(env, d_act, 1.0f, n);
    env.SetActorExploration(GYMNET_ACTOR_EXPLORE_SOFTMAX, 0.5f);
    env.GetActorExploration(explore, temperature);
    CHECK(explore == GYMNET_ACTOR_EXPLORE_SOFTMAX && temperature == 0.5f, "round trip");
    const std::vector<int32_t> drawn = act(env, d_act, 1.0f, n);
    int ones = 0;
    for (int32_t a : drawn) ones += a == 1;
    CHECK(drawn == uniform, "equal logits, two actions: floor(2 u) is the uniform draw");
    CHECK(ones > n / 4 && ones < 3 * n / 4, "both actions occur");
    const std::vector<int32_t> greedy = act(env, d_act, 0.0f, n);
    bool first = true;
    for (int32_t a : greedy) first &= a == 0;
    CHECK(first, "epsilon 0: the argmax, the first of two equal logits");

    const float bad[5] = {std::numeric_limits<float>::quiet_NaN(), 0.0f, -1.0f, std::numeric_limits<float>::infinity(), 1e-39f};
    for (float t : bad) CHECK(gymnet_vecenv_actor_set_exploration(env.handle(), GYMNET_ACTOR_EXPLORE_SOFTMAX, t) == GYMNET_ERR_INVALID_ARG, "temperature");
    CHECK(gymnet_vecenv_actor_set_exploration(env.handle(), 2, 1.0f) == GYMNET_ERR_INVALID_ARG, "explore");
    CHECK(gymnet_vecenv_actor_set_exploration(env.handle(), -1, 1.0f) == GYMNET_ERR_INVALID_ARG, "explore");
    bool refused = false;
    try { env.SetActorExploration((gymnet_actor_explore)7); } catch (const std::exception &) { refused = true; }
    CHECK(refused, "the wrapper throws on a refusal");
    env.GetActorExploration(explore, temperature);
    CHECK(explore == GYMNET_ACTOR_EXPLORE_SOFTMAX && temperature == 0.5f, "refusals leave the setting");
    CHECK(act(env, d_act, 1.0f, n) == drawn, "... and the actions");

    CHECK(hipMemcpy(d_w, apart.data(), sizeof(float) * apart.size(), hipMemcpyHostToDevice) == hipSuccess, "copy");
    env.LoadActorWeights(d_w, (int64_t)apart.size());
    env.GetActorExploration(explore, temperature);
    CHECK(explore == GYMNET_ACTOR_EXPLORE_SOFTMAX && temperature == 0.5f, "a load keeps the setting");
    const std::vector<int32_t> sure = act(env, d_act, 1.0f, n);
    bool all_one = true;
    for (int32_t a : sure) all_one &= a == 1;
    CHECK(all_one, "a gap of 1000: the far action has weight 0 and no lane takes it");
    env.SetActorExploration(GYMNET_ACTOR_EXPLORE_UNIFORM, 0.5f);
    CHECK(act(env, d_act, 1.0f, n) == uniform, "UNIFORM again: the uniform draw, whatever the logits and the temperature");
    env.SetActorExploration(GYMNET_ACTOR_EXPLORE_SOFTMAX, 0.5f);

    env.StepDevice(d_act);                                      // the fused rollout's unfused counterpart
    env.PushActor();
    env.GetActorExploration(explore, temperature);
    CHECK(explore == GYMNET_ACTOR_EXPLORE_SOFTMAX && temperature == 0.5f, "a push keeps the setting");
    env.ConfigureActor(1, {4, 2}, equal);
    env.GetActorExploration(explore, temperature);
    CHECK(explore == GYMNET_ACTOR_EXPLORE_UNIFORM && temperature == 1.0f, "a re-config returns to the default");
    env.ConfigureActor(0, {}, {});
    (void)hipFree(d_act);
    (void)hipFree(d_w);

    gymnet::VectorEnv box(GYMNET_ENV_PENDULUM, n, 0, 7, 0);      // a Box actor is refused, and the message says so
    box.Reset();
    box.ConfigureBoxActor(1, {3, 1}, {0.0f, 0.0f, 1.0f, 0.0f});
    int32_t ex = -9;
    float tp = -9.0f;
    CHECK(gymnet_vecenv_actor_set_exploration(box.handle(), GYMNET_ACTOR_EXPLORE_SOFTMAX, 1.0f) == GYMNET_ERR_INVALID_ARG, "a Box actor");
    CHECK(std::string(gymnet_last_error()).find("Box") != std::string::npos, "the message names Box");
    CHECK(gymnet_vecenv_actor_get_exploration(box.handle(), &ex, &tp) == GYMNET_ERR_INVALID_ARG && ex == -9 && tp == -9.0f, "outputs untouched");
    box.ConfigureBoxActor(0, {}, {});
}
#endif

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
#ifdef SOFTMAX_STUB
    stub_checks();
    std::printf("stub: %d failed\n", failed);
#else
    cpu_checks(mode == "--gpu");
    if (mode == "--gpu") gpu_checks();
    std::printf("%s: %d failed\n", mode == "--gpu" ? "cpu+gpu" : "cpu", failed);
#endif
    return failed ? 1 : 0;
}
