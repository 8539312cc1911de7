// pixel_stack_test.cpp — the C++ host side of the pixel frame stacks (gymnet::VectorEnv::ConfigurePixelStack / PushPixelStack /
// ReadPixelStack in include/gymnet_amd.hpp), built with g++ against libgymnet_amd.so.
//   --cpu: the calls refuse a null handle and write nothing; no GPU needed.
//   --gpu: a CartPole handle with auto-reset keeps the Images runner's stack (two 40 x 20 GRAY8 frames): after config both slots hold the
//          rendered frame, after a step the older slot holds the previous frame and the newer the new one, and a lane that finished
//          holds its new frame in both.
#include <cstdio>
#include <cstring>
#include <vector>

#include "gymnet_amd.hpp"

static int failed = 0;
#define CHECK(cond, msg)                                                          \
    do {                                                                          \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, msg); ++failed; } \
    } while (0)

static std::vector<uint8_t> render_gray(gymnet_vecenv *h, int64_t n) {
    std::vector<uint8_t> f((size_t)n * 800);
    gymnet::check(gymnet_vecenv_render(h, f.data(), GYMNET_PIXELS_GRAY8, 0, n, 200, 150, 200, 150, 40, 20, 800));
    return f;
}

static void cpu_checks() {
    uint8_t buf[64];
    std::memset(buf, 0x5A, sizeof buf);
    CHECK(gymnet_vecenv_pixel_stack_config(nullptr, GYMNET_STACK_GRAY8, 2, 200, 150, 200, 150, 40, 20, nullptr, 0) == GYMNET_ERR_INVALID_ARG, "config");
    CHECK(gymnet_vecenv_pixel_stack_push_device(nullptr, nullptr) == GYMNET_ERR_INVALID_ARG, "push");
    CHECK(gymnet_vecenv_pixel_stack_reset_device(nullptr, nullptr) == GYMNET_ERR_INVALID_ARG, "reset");
    CHECK(gymnet_vecenv_pixel_stack_view(nullptr, nullptr, nullptr, nullptr) == GYMNET_ERR_INVALID_ARG, "view");
    CHECK(gymnet_vecenv_pixel_stack_read(nullptr, buf, 0, 1) == GYMNET_ERR_INVALID_ARG, "read");
    bool untouched = true;
    for (uint8_t b : buf) untouched &= b == 0x5A;
    CHECK(untouched, "nothing written");
}

static void gpu_checks() {
    const int64_t n = 512;
    gymnet::VectorEnv env(GYMNET_ENV_CARTPOLE, n, 0, 7, GYMNET_FLAG_AUTORESET);
    env.Reset();
    env.ConfigurePixelStack(GYMNET_STACK_GRAY8, 2, 40, 20, 200, 150, 200, 150);
    const auto v = env.PixelStack();
    CHECK(v.d_stack != nullptr && v.lane_stride == 1600 && v.frame_bytes == 800, "view");
    std::vector<uint8_t> s0 = env.ReadPixelStack<uint8_t>();
    CHECK(s0.size() == (size_t)n * 1600, "size");
    // the same frames through the C ABI, on a twin handle in the same state
    gymnet_vecenv *h = nullptr;
    gymnet_config cfg{};
    cfg.struct_size = sizeof cfg; cfg.env_id = GYMNET_ENV_CARTPOLE; cfg.num_envs = n; cfg.seed = 7; cfg.flags = GYMNET_FLAG_AUTORESET;
    gymnet::check(gymnet_vecenv_create(&cfg, &h));
    std::vector<float> obs0((size_t)n * 4);
    gymnet::check(gymnet_vecenv_reset(h, obs0.data()));
    std::vector<uint8_t> f0 = render_gray(h, n);
    bool ok = true;
    for (int64_t k = 0; k < n; ++k)
        ok &= std::memcmp(&s0[(size_t)k * 1600], &f0[(size_t)k * 800], 800) == 0 && std::memcmp(&s0[(size_t)k * 1600 + 800], &f0[(size_t)k * 800], 800) == 0;
    CHECK(ok, "config fills both slots with the rendered frame");
    // steps with the same actions on both handles; the stack shifts, finished lanes restart
    int64_t restarted = 0;
    std::vector<uint8_t> prev = f0;
    for (int t = 0; t < 30; ++t) {
        std::vector<int> a((size_t)n);
        for (int64_t k = 0; k < n; ++k) a[(size_t)k] = (int)((k * 7 + t * 3) % 2);
        auto b = env.Step(a);
        env.PushPixelStack();
        std::vector<float> obs((size_t)n * 4), rew((size_t)n);
        std::vector<uint8_t> done((size_t)n);
        gymnet::check(gymnet_vecenv_step(h, a.data(), obs.data(), rew.data(), done.data()));
        std::vector<uint8_t> cur = render_gray(h, n);
        std::vector<uint8_t> st = env.ReadPixelStack<uint8_t>();
        for (int64_t k = 0; k < n; ++k) {
            const uint8_t *older = done[(size_t)k] ? &cur[(size_t)k * 800] : &prev[(size_t)k * 800];
            ok &= std::memcmp(&st[(size_t)k * 1600], older, 800) == 0 && std::memcmp(&st[(size_t)k * 1600 + 800], &cur[(size_t)k * 800], 800) == 0;
            ok &= (b.Done[(size_t)k] != 0) == (done[(size_t)k] != 0);
            restarted += done[(size_t)k];
        }
        prev = cur;
    }
    CHECK(ok, "push: older slot = previous frame (restart: the new one), newer slot = the new frame");
    CHECK(restarted > 0, "some lanes finished");
    std::vector<uint8_t> part = env.ReadPixelStack<uint8_t>(5, 3);
    std::vector<uint8_t> all = env.ReadPixelStack<uint8_t>();
    CHECK(part.size() == 3 * 1600 && std::memcmp(part.data(), &all[5 * 1600], part.size()) == 0, "lane range");
    CHECK([&] { try { env.ReadPixelStack<uint8_t>(n, 1); return false; } catch (const std::invalid_argument &) { return true; } }(), "lanes outside");
    env.ConfigurePixelStack(GYMNET_STACK_BINARY_F32, 2);
    std::vector<float> fs = env.ReadPixelStack<float>();
    std::vector<uint8_t> g = render_gray(h, n);
    ok = fs.size() == (size_t)n * 1600;
    for (int64_t k = 0; ok && k < n; ++k)
        for (int p = 0; p < 800; ++p) ok &= fs[(size_t)k * 1600 + 800 + p] == (g[(size_t)k * 800 + p] < 255 ? 1.0f : 0.0f);
    CHECK(ok, "BINARY_F32 = (gray < 255) as float");
    gymnet::check(gymnet_vecenv_destroy(h));
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
