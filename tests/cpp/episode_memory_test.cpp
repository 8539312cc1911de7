// episode_memory_test.cpp — the C++ host side of the episode memory (gymnet::VectorEnv::ConfigureEpisodeMemory / PushEpisodeMemory /
// ReadMemoryEpisodes / BuildMemoryDataset in include/gymnet_amd.hpp), built with g++ against libgymnet_amd.so and the HIP runtime.
//   --cpu: the calls refuse a null handle and write nothing; no GPU needed.
//   --gpu: a CartPole auto-reset handle (max_length 500), sampled actions drawn on the device: the kept set is the best episodes in
//          descending key order (every CartPole reward is 1, so return == length), its size is min(capacity, ended), and the params
//          dataset has floor(len * 2 / 3) rows per episode whose one-hot matches the action and whose first row repeats o_0.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "gymnet_amd.hpp"

static int failed = 0;
#define CHECK(cond, msg)                                                          \
    do {                                                                          \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, msg); ++failed; } \
    } while (0)

static void cpu_checks() {
    int64_t v[4] = {-7, -7, -7, -7};
    float r[2] = {-7.0f, -7.0f};
    CHECK(gymnet_vecenv_memory_config(nullptr, 100, 0, 4) == GYMNET_ERR_INVALID_ARG, "config");
    CHECK(gymnet_vecenv_memory_reset_device(nullptr, nullptr, 0) == GYMNET_ERR_INVALID_ARG, "reset");
    CHECK(gymnet_vecenv_memory_push_device(nullptr, r, nullptr) == GYMNET_ERR_INVALID_ARG, "push");
    CHECK(gymnet_vecenv_memory_stats(nullptr, &v[0], &v[1], &v[2], &v[3]) == GYMNET_ERR_INVALID_ARG, "stats");
    CHECK(gymnet_vecenv_memory_episodes(nullptr, r, nullptr, nullptr, nullptr, 2, &v[0]) == GYMNET_ERR_INVALID_ARG, "episodes");
    CHECK(gymnet_vecenv_memory_dataset_size(nullptr, &v[0]) == GYMNET_ERR_INVALID_ARG, "size");
    CHECK(gymnet_vecenv_memory_dataset_device(nullptr, GYMNET_MEMORY_PARAMS, 0, 0, 0, 0, 0, 0, r, nullptr, nullptr, nullptr, 1) ==
          GYMNET_ERR_INVALID_ARG, "dataset");
    CHECK(v[0] == -7 && v[1] == -7 && v[2] == -7 && v[3] == -7 && r[0] == -7.0f && r[1] == -7.0f, "nothing written");
}

static void gpu_checks() {
    const int64_t n = 1024;
    const int32_t capacity = 16, history = 4;
    gymnet::VectorEnv env(GYMNET_ENV_CARTPOLE, n, 0, 7, GYMNET_FLAG_AUTORESET);
    env.Reset();
    env.ConfigureEpisodeMemory(capacity, 500, history);
    CHECK(env.BuildMemoryDataset(nullptr, nullptr, nullptr, 0, capacity) == -1, "no dataset before the memory holds capacity episodes");
    int32_t *d_act = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_act), sizeof(int32_t) * n) == hipSuccess, "hipMalloc");
    for (int t = 0; t < 80; ++t) {
        gymnet::check(gymnet_vecenv_sample_actions_device(env.handle(), d_act, 11, (uint64_t)t));
        env.StepDevice(d_act);
        env.PushEpisodeMemory(d_act);
    }
    bool refused = false;
    try { env.PushEpisodeMemory(d_act); } catch (const std::exception &) { refused = true; }
    CHECK(refused, "a second push without a step is refused");
    const auto st = env.EpisodeMemoryStats();
    const auto ep = env.ReadMemoryEpisodes();
    CHECK(st.ended > capacity && st.kept == capacity && (int64_t)ep.ret.size() == capacity && st.too_long == 0, "kept = min(capacity, ended)");
    bool ordered = true;
    int64_t rows = 0;
    for (size_t i = 0; i < ep.ret.size(); ++i) {
        ordered &= ep.ret[i] == (float)ep.len[i] && ep.len[i] <= 500;
        if (i > 0) ordered &= ep.ret[i] < ep.ret[i - 1] || (ep.ret[i] == ep.ret[i - 1] && (ep.end_tick[i] < ep.end_tick[i - 1] ||
                              (ep.end_tick[i] == ep.end_tick[i - 1] && ep.lane[i] < ep.lane[i - 1])));
        rows += (int64_t)ep.len[i] * 2 / 3;
    }
    CHECK(ordered, "descending (return, end tick, lane), return == length");
    CHECK(env.MemoryDatasetRows() == rows, "rows = sum of floor(len * 2 / 3)");
    float *d_x = nullptr, *d_onehot = nullptr;
    int32_t *d_a = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_x), sizeof(float) * rows * history * 4) == hipSuccess, "hipMalloc x");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_onehot), sizeof(float) * rows * 2) == hipSuccess, "hipMalloc onehot");
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_a), sizeof(int32_t) * rows) == hipSuccess, "hipMalloc action");
    CHECK(env.BuildMemoryDataset(d_x, d_a, d_onehot, rows, capacity) == rows, "rows written");
    env.Sync();
    std::vector<float> x((size_t)rows * history * 4), oh((size_t)rows * 2);
    std::vector<int32_t> a((size_t)rows);
    CHECK(hipMemcpy(x.data(), d_x, x.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess, "copy x");
    CHECK(hipMemcpy(oh.data(), d_onehot, oh.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess, "copy onehot");
    CHECK(hipMemcpy(a.data(), d_a, a.size() * sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess, "copy action");
    bool ok = true;
    for (int64_t r = 0; r < rows; ++r) ok &= (a[(size_t)r] == 0 || a[(size_t)r] == 1) && oh[(size_t)r * 2 + a[(size_t)r]] == 1.0f &&
                                            oh[(size_t)r * 2 + 1 - a[(size_t)r]] == 0.0f;
    CHECK(ok, "one-hot of the action");
    for (int s = 1; s < history; ++s) ok &= std::memcmp(&x[0], &x[(size_t)s * 4], 4 * sizeof(float)) == 0;
    CHECK(ok, "the first row repeats o_0 in every history slot");
    (void)hipFree(d_act); (void)hipFree(d_x); (void)hipFree(d_onehot); (void)hipFree(d_a);
}

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::strcmp(argv[1], "--gpu") == 0;
    cpu_checks();
    if (gpu) {
        try {
            gpu_checks();
        } catch (const std::exception &e) {
            std::printf("FAIL exception: %s\n", e.what());
            ++failed;
        }
    }
    std::printf("%s: %d failed\n", gpu ? "cpu+gpu" : "cpu", failed);
    return failed ? 1 : 0;
}
