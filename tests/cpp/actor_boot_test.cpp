// actor_boot_test.cpp — the C++ host side of V(terminal observation) on time-limit rows (gymnet::VectorEnv::ActorBoot /
// RolloutFusedValueBoot / RolloutFusedBoxBoot in include/gymnet_amd.hpp).
//   --stub: built with -DBOOT_STUB against tests/cpp/abi_stub.c and tests/cpp/actor_boot_stub.c, under the sanitizers: the three methods
//           hand their arguments across unchanged into buffers of exactly the documented sizes, set struct_size, forward on a null boot
//           pointer, and throw on a refusal that writes nothing.
//   --cpu:  built against libgymnet_amd.so: the three calls refuse a null handle, also when they forward, and write nothing; no GPU needed.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "gymnet_amd.hpp"

static int failed = 0;
#define CHECK(cond, msg)                                                          \
    do {                                                                          \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, msg); ++failed; } \
    } while (0)

#ifdef BOOT_STUB
extern "C" {
typedef struct boot_stub_call {
    int calls, forwarded;
    int log[16];
    float epsilon; uint64_t seed, tick;
    int64_t steps; int32_t action_source;
    const float *lp_at, *value_at, *boot_at;
} boot_stub_call;
const boot_stub_call *boot_stub_last(void);
void boot_stub_setup(int64_t n, int critic, int max_episode_steps);
void boot_stub_clear(void);
void boot_stub_stepped(void);
void boot_stub_pushed(void);
}

template <class F>
static bool throws(F f) {
    try { f(); } catch (const std::exception &) { return true; }
    return false;
}

static void stub_checks() {
    const int64_t n = 37, T = 3;
    gymnet::VectorEnv env(GYMNET_ENV_CARTPOLE, n);
    boot_stub_clear();
    boot_stub_setup(n, 1, 7);
    const boot_stub_call *c = boot_stub_last();
    std::vector<float> boot((size_t)n, -7.0f);                                  // exactly the documented size
    CHECK(throws([&] { env.ActorBoot(boot.data()); }) && c->calls == 0 && boot[1] == -7.0f, "no step since the push: throws, writes nothing");
    boot_stub_stepped();
    env.ActorBoot(boot.data());
    CHECK(c->calls == 1 && c->log[0] == 1 && c->boot_at == boot.data(), "the pointer crosses");
    CHECK(boot[0] == 0.0f && boot[(size_t)n - 1] == 0.0f && boot[(size_t)n - 2] == 2000.0f + (float)(n - 2), "every lane written: a value or +0");
    CHECK(throws([&] { env.ActorBoot(nullptr); }) && c->calls == 1, "a null pointer throws");
    boot_stub_setup(n, 1, 0);
    CHECK(throws([&] { env.ActorBoot(boot.data()); }) && c->calls == 1, "no time limit throws");
    boot_stub_setup(n, 0, 7);
    CHECK(throws([&] { env.ActorBoot(boot.data()); }) && c->calls == 1, "no critic throws");
    boot_stub_setup(n, 1, 7);

    std::vector<float> rec_lp((size_t)(T * n), 1.0f), rec_value((size_t)(T * n), 1.0f), rec_boot((size_t)(T * n), 1.0f);
    gymnet_rollout_spec spec{};
    spec.action_source = GYMNET_ACTIONS_ACTOR; spec.steps = T; spec.epsilon = 0.75f; spec.action_seed = 9; spec.action_tick0 = 100;
    env.RolloutFusedValueBoot(spec, rec_lp.data(), rec_value.data(), rec_boot.data());     // (struct_size is the wrapper's to set: the stub refuses any other)
    CHECK(c->calls == 2 && c->log[1] == 2 && c->forwarded == 0 && c->steps == T && c->action_source == GYMNET_ACTIONS_ACTOR, "the spec crosses");
    CHECK(c->epsilon == 0.75f && c->seed == 9 && c->tick == 100, "... with its action stream");
    CHECK(c->lp_at == rec_lp.data() && c->value_at == rec_value.data() && c->boot_at == rec_boot.data(), "the three pointers cross, in their order");
    const size_t last = (size_t)(T * n - 1);
    CHECK(rec_lp[last] == -(float)last && rec_value[last] == (float)last && rec_boot[last - 1] == 2000.0f + (float)(last - 1) && rec_boot[last] == 0.0f, "every row written");
    std::fill(rec_boot.begin(), rec_boot.end(), 1.0f);
    env.RolloutFusedValueBoot(spec, nullptr, rec_value.data(), rec_boot.data());
    CHECK(c->calls == 3 && c->lp_at == nullptr && rec_boot[1] == 2001.0f, "without logp");
    env.RolloutFusedValueBoot(spec, rec_lp.data(), rec_value.data(), nullptr);
    CHECK(c->calls == 4 && c->forwarded == 1 && c->boot_at == nullptr, "a null boot forwards");
    std::fill(rec_boot.begin(), rec_boot.end(), 1.0f);
    std::fill(rec_value.begin(), rec_value.end(), 1.0f);
    CHECK(throws([&] { env.RolloutFusedValueBoot(spec, rec_lp.data(), nullptr, rec_boot.data()); }) && c->calls == 4 && rec_boot[1] == 1.0f,
          "a boot without the values throws and writes nothing");
    boot_stub_setup(n, 1, 0);
    CHECK(throws([&] { env.RolloutFusedValueBoot(spec, nullptr, rec_value.data(), rec_boot.data()); }) && c->calls == 4 && rec_value[1] == 1.0f && rec_boot[1] == 1.0f,
          "no time limit throws and writes nothing");
    boot_stub_setup(n, 1, 7);

    env.RolloutFusedBoxBoot(spec, rec_lp.data(), rec_value.data(), rec_boot.data());
    CHECK(c->calls == 5 && c->log[4] == 3 && c->lp_at == rec_lp.data() && c->value_at == rec_value.data() && c->boot_at == rec_boot.data(), "the Box call: three pointers");
    CHECK(rec_boot[last - 1] == 2000.0f + (float)(last - 1) && rec_value[last] == (float)last, "... written");
    env.RolloutFusedBoxBoot(spec, nullptr, rec_value.data(), nullptr);
    CHECK(c->calls == 6 && c->forwarded == 2, "a null boot forwards there too");
    spec.action_source = GYMNET_ACTIONS_SAMPLE;
    std::fill(rec_boot.begin(), rec_boot.end(), 1.0f);
    CHECK(throws([&] { env.RolloutFusedBoxBoot(spec, nullptr, rec_value.data(), rec_boot.data()); }) && c->calls == 6 && rec_boot[1] == 1.0f,
          "a source other than the actor throws and writes nothing");
}
#else
static void cpu_checks() {
    float value[2] = {1.0f, 1.0f}, boot[2] = {-7.0f, -7.0f};
    gymnet_rollout_spec spec{};
    spec.struct_size = sizeof spec; spec.action_source = GYMNET_ACTIONS_ACTOR; spec.steps = 1;
    CHECK(gymnet_vecenv_actor_boot_device(nullptr, boot) == GYMNET_ERR_INVALID_ARG, "boot: null handle");
    CHECK(gymnet_vecenv_rollout_fused_value_boot_device(nullptr, &spec, nullptr, value, boot) == GYMNET_ERR_INVALID_ARG, "rollout_fused_value_boot: null handle");
    CHECK(gymnet_vecenv_rollout_fused_value_boot_device(nullptr, &spec, nullptr, value, nullptr) == GYMNET_ERR_INVALID_ARG, "... also when it forwards");
    CHECK(gymnet_vecenv_rollout_fused_value_boot_device(nullptr, &spec, nullptr, nullptr, nullptr) == GYMNET_ERR_INVALID_ARG, "... all the way");
    CHECK(gymnet_vecenv_rollout_fused_box_boot_device(nullptr, &spec, nullptr, value, boot) == GYMNET_ERR_INVALID_ARG, "rollout_fused_box_boot: null handle");
    CHECK(gymnet_vecenv_rollout_fused_box_boot_device(nullptr, &spec, nullptr, nullptr, nullptr) == GYMNET_ERR_INVALID_ARG, "... also when it forwards");
    CHECK(value[0] == 1.0f && value[1] == 1.0f && boot[0] == -7.0f && boot[1] == -7.0f, "nothing written");
    CHECK(GYMNET_ABI_VERSION == 6, "ABI 6");
}
#endif

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    (void)mode;
#ifdef BOOT_STUB
    stub_checks();
    std::printf("stub: %d failed\n", failed);
#else
    cpu_checks();
    std::printf("cpu: %d failed\n", failed);
#endif
    return failed ? 1 : 0;
}
