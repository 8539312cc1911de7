// episode_memory_rollout_test.cpp — the C++ host side of the episode memory's rollout ingest (gymnet::VectorEnv::
// ConfigureEpisodeMemoryRollout / PushMemoryRollout in include/gymnet_amd.hpp).
//   --stub: built with -DROLLOUT_STUB against tests/cpp/abi_stub.c and tests/cpp/episode_memory_rollout_stub.c, under the sanitizers: the
//           two methods hand their arguments across unchanged, the defaults are action_stride = N and ring = steps, the buffers have the
//           documented sizes (the stub reads every byte of them), a refusal throws.
//   --cpu:  built against libgymnet_amd.so: the two calls refuse a null handle; no GPU needed.
//   --gpu:  twin CartPole handles with auto-reset, 300 lanes, episodes of up to 30 steps kept: A runs T x (StepDevice, PushEpisodeMemory), B one fused
//           rollout that records, then PushMemoryRollout; stats and kept episodes are equal, and the single push stays refused on B.
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

#ifdef ROLLOUT_STUB
extern "C" {
typedef struct rollout_stub_call {
    int calls;
    int32_t capacity, max_length, history, rollout_chunk;
    int64_t steps, action_stride, ring;
    const void *rec_obs, *actions, *rec_reward, *rec_done;
} rollout_stub_call;
void rollout_stub_shape(int64_t n, int obs_dim);
const rollout_stub_call *rollout_stub_last(void);
}

static void stub_checks() {
    const int64_t n = 37, steps = 9;
    gymnet::VectorEnv env(GYMNET_ENV_CARTPOLE, n);
    rollout_stub_shape(n, env.ObsDim());
    env.ConfigureEpisodeMemoryRollout(7, 11, 3, 16);
    const rollout_stub_call *c = rollout_stub_last();
    CHECK(c->calls == 1 && c->capacity == 7 && c->max_length == 11 && c->history == 3 && c->rollout_chunk == 16, "config arguments");
    env.ConfigureEpisodeMemoryRollout();
    CHECK(c->calls == 2 && c->capacity == 100 && c->max_length == 0 && c->history == 4 && c->rollout_chunk == 16, "config defaults");
    bool refused = false;
    try { env.ConfigureEpisodeMemoryRollout(7, 11, 3, 65); } catch (const std::exception &) { refused = true; }
    CHECK(refused && c->calls == 2, "a refused config throws");
    std::vector<float> obs((size_t)(steps * env.ObsDim() * n)), rew((size_t)(steps * n));
    std::vector<uint8_t> done((size_t)(steps * n));
    std::vector<int32_t> rec_actions((size_t)(steps * n)), ring((size_t)(2 * n));
    env.PushMemoryRollout(steps, obs.data(), rec_actions.data(), rew.data(), done.data());
    CHECK(c->calls == 3 && c->steps == steps && c->action_stride == n && c->ring == steps, "defaults: a [steps][N] record");
    CHECK(c->rec_obs == obs.data() && c->actions == rec_actions.data() && c->rec_reward == rew.data() && c->rec_done == done.data(), "pointers");
    env.PushMemoryRollout(steps, obs.data(), ring.data(), rew.data(), done.data(), n, 2);
    CHECK(c->calls == 4 && c->action_stride == n && c->ring == 2 && c->actions == ring.data(), "a ring of 2 rows");
    env.PushMemoryRollout(steps, obs.data(), ring.data(), rew.data(), done.data(), 0, 1);
    CHECK(c->calls == 5 && c->action_stride == 0 && c->ring == 1, "one broadcast row");
    refused = false;
    try { env.PushMemoryRollout(0, obs.data(), ring.data(), rew.data(), done.data()); } catch (const std::exception &) { refused = true; }
    CHECK(refused && c->calls == 5, "steps 0 throws");
    refused = false;
    try { env.PushMemoryRollout(steps, nullptr, ring.data(), rew.data(), done.data()); } catch (const std::exception &) { refused = true; }
    CHECK(refused && c->calls == 5, "a null buffer throws");
}
#else
#include <hip/hip_runtime_api.h>

static void cpu_checks() {
    int dummy = 0;
    CHECK(gymnet_vecenv_memory_config_rollout(nullptr, 100, 0, 4, 16) == GYMNET_ERR_INVALID_ARG, "config_rollout on a null handle");
    CHECK(gymnet_vecenv_memory_push_rollout_device(nullptr, 1, &dummy, &dummy, 0, 1, reinterpret_cast<const float *>(&dummy),
                                                   reinterpret_cast<const uint8_t *>(&dummy)) == GYMNET_ERR_INVALID_ARG, "push_rollout on a null handle");
    CHECK(dummy == 0, "nothing written");
    CHECK(GYMNET_ABI_VERSION == 6, "ABI 6");
}

template <class T>
static T *dev(size_t count) {
    T *p = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void **>(&p), sizeof(T) * count) == hipSuccess, "hipMalloc");
    return p;
}

static void gpu_checks() {
    const int64_t n = 300, T = 40;
    std::vector<int32_t> actions((size_t)(T * n));
    uint32_t x = 12345u;
    for (auto &a : actions) { x = x * 1664525u + 1013904223u; a = (int32_t)((x >> 16) & 1u); }
    int32_t *d_ring = dev<int32_t>((size_t)(T * n));
    CHECK(hipMemcpy(d_ring, actions.data(), sizeof(int32_t) * actions.size(), hipMemcpyHostToDevice) == hipSuccess, "copy");
    float *d_obs = dev<float>((size_t)(T * 4 * n)), *d_rew = dev<float>((size_t)(T * n));
    uint8_t *d_done = dev<uint8_t>((size_t)(T * n));
    gymnet::VectorEnv::MemoryStats stats[2];
    gymnet::VectorEnv::MemoryEpisodes eps[2];
    for (int fused = 0; fused < 2; ++fused) {
        gymnet::VectorEnv env(GYMNET_ENV_CARTPOLE, n, 0, 7, GYMNET_FLAG_AUTORESET);
        env.Reset();
        if (fused) env.ConfigureEpisodeMemoryRollout(5, 30, 2, 16); else env.ConfigureEpisodeMemory(5, 30, 2);
        if (fused) {
            gymnet_rollout_buffers rec{d_obs, d_rew, d_done};
            gymnet::check(gymnet_vecenv_rollout_fused_device(env.handle(), d_ring, T, n, T, &rec));
            env.PushMemoryRollout(T, d_obs, d_ring, d_rew, d_done);
            CHECK(gymnet_vecenv_memory_push_device(env.handle(), d_ring, nullptr) == GYMNET_ERR_INVALID_ARG, "the single push stays refused");
            CHECK(gymnet_vecenv_memory_push_rollout_device(env.handle(), T, d_obs, d_ring, n, T, d_rew, d_done) == GYMNET_ERR_INVALID_ARG, "a second ingest");
        } else {
            for (int64_t t = 0; t < T; ++t) { env.StepDevice(d_ring + t * n); env.PushEpisodeMemory(d_ring + t * n); }
        }
        stats[fused] = env.EpisodeMemoryStats();
        eps[fused] = env.ReadMemoryEpisodes();
        env.ConfigureEpisodeMemory(0);
    }
    CHECK(stats[0].ended > 5 && stats[0].kept == 5 && stats[0].admitted > 5, "the pool overflowed");
    CHECK(stats[0].kept == stats[1].kept && stats[0].ended == stats[1].ended && stats[0].admitted == stats[1].admitted &&
          stats[0].too_long == stats[1].too_long, "stats");
    CHECK(eps[0].ret == eps[1].ret && eps[0].len == eps[1].len && eps[0].end_tick == eps[1].end_tick && eps[0].lane == eps[1].lane, "kept episodes");
    (void)hipFree(d_ring); (void)hipFree(d_obs); (void)hipFree(d_rew); (void)hipFree(d_done);
}
#endif

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
#ifdef ROLLOUT_STUB
    stub_checks();
    std::printf("stub: %d failed\n", failed);
#else
    cpu_checks();
    if (mode == "--gpu") gpu_checks();
    std::printf("%s: %d failed\n", mode == "--gpu" ? "cpu+gpu" : "cpu", failed);
#endif
    return failed ? 1 : 0;
}
