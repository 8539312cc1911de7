// advantage_test.cpp — the C++ host side of the advantage / return call: gymnet::VectorEnv::AdvantagesDevice (include/gymnet_amd.hpp) and
// the form picker pick_advantage_form (gym.net_amd/csrc/advantage.hpp, host-only and pure).
//   --stub: built with -DADVANTAGE_STUB against tests/cpp/abi_stub.c and tests/cpp/advantage_stub.c, under the sanitizers: the picker's
//           boundaries, and the wrapper handing device, stream, sizes (count = stride = N) and pointers across unchanged into buffers of
//           exactly the documented sizes, with its defaults, both in-place forms, a NULL output, and a refusal that throws.
//   --cpu:  built against libgymnet_amd.so: the picker again, and everything gymnet_gae_device refuses or skips before it touches the
//           device (bad sizes, gamma, lambda, NULL and aliased pointers; steps or count 0 is a no-op); no GPU needed.
//   --gpu:  a CartPole handle of 260 lanes, T = 17: the wrapper's result on device buffers equals the recurrence run on the host, bit for
//           bit, with and without values and boot, and in place.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "advantage.hpp"
#include "gymnet_amd.hpp"

static int failed = 0;
#define CHECK(cond, msg)                                                          \
    do {                                                                          \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, msg); ++failed; } \
    } while (0)

// the header's recurrence on host memory (the reference of the --stub and --gpu legs)
static void recurrence(int64_t T, int64_t n, const float *r, const uint8_t *d, const float *v, const float *vlast, const float *boot, float gamma,
                       float lambda, float *adv, float *ret) {
    const float gl = gamma * lambda;
    for (int64_t i = 0; i < n; ++i) {
        float A = 0.0f, vnext = vlast ? vlast[i] : 0.0f;
        for (int64_t t = T - 1; t >= 0; --t) {
            const int64_t k = t * n + i;
            const float vk = v ? v[k] : 0.0f;
            const float nv = (d[k] & 1) ? 0.0f : (d[k] & 2) ? (boot ? boot[k] : 0.0f) : vnext;
            const float delta = std::fmaf(gamma, nv, r[k]) - vk;
            A = d[k] ? delta : std::fmaf(gl, A, delta);
            if (adv) adv[k] = A;
            if (ret) ret[k] = A + vk;
            vnext = vk;
        }
    }
}

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

struct Inputs {
    int64_t T, n;
    std::vector<float> r, v, vlast, boot;
    std::vector<uint8_t> d;
    Inputs(int64_t T_, int64_t n_) : T(T_), n(n_), r((size_t)(T_ * n_)), v((size_t)(T_ * n_)), vlast((size_t)n_), boot((size_t)(T_ * n_)), d((size_t)(T_ * n_)) {
        uint32_t s = 12345u;
        auto next = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
        for (size_t k = 0; k < r.size(); ++k) {
            r[k] = (float)(next() % 2001) / 1000.0f - 1.0f;
            v[k] = (float)(next() % 2001) / 500.0f - 2.0f;
            boot[k] = (float)(next() % 2001) / 250.0f - 4.0f;
            d[k] = next() % 10 == 0 ? (uint8_t)(1 + next() % 3) : (uint8_t)0;
        }
        for (auto &x : vlast) x = (float)(next() % 2001) / 500.0f - 2.0f;
        d[0] = 2; d[(size_t)((T - 1) * n + n - 1)] = 1;             // a done on row 0 and on row T-1
    }
};

static void picker_checks() {
    using gymnet::AdvantagePointers;
    // the alignment and divisibility rules, with the small-batch threshold out of the way (narrow_below = 0) ...
    auto pick_advantage_form = [](int64_t count, int64_t stride, const AdvantagePointers &p) { return gymnet::pick_advantage_form(count, stride, p, 0); };
    const AdvantagePointers all{0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000};
    gymnet::AdvantageForm f = pick_advantage_form(1028, 1028, all);
    CHECK(f.vec == 4 && f.has_value && f.has_boot && f.threads == 257 && f.blocks == 2, "aligned, divisible: V = 4, a second block of one thread");
    f = pick_advantage_form(1028, 1040, all);
    CHECK(f.vec == 4 && f.threads == 257, "stride = n + 12: V = 4 survives");
    for (int64_t pad : {1, 2, 3, 5}) CHECK(pick_advantage_form(1028, 1028 + pad, all).vec == 1, "stride % 4 != 0: V = 1");
    for (int64_t n : {1, 3, 5, 1030}) {
        f = pick_advantage_form(n, 1032, all);
        CHECK(f.vec == 1 && f.threads == n && f.blocks == (n + 255) / 256, "count % 4 != 0: V = 1, one thread per lane");
    }
    f = pick_advantage_form(4, 4, all);
    CHECK(f.vec == 4 && f.threads == 1 && f.blocks == 1, "n = 4: a single thread");
    f = pick_advantage_form(0, 0, all);
    CHECK(f.threads == 0 && f.blocks == 0, "n = 0: nothing to launch");
    f = pick_advantage_form(252, 252, all);
    CHECK(f.vec == 4 && f.threads == 63 && f.blocks == 1, "n = 252: a partial wave");
    // each float pointer's 16-byte boundary and the done pointer's 4-byte boundary, one at a time
    uintptr_t AdvantagePointers::*floats[] = {&AdvantagePointers::reward, &AdvantagePointers::value, &AdvantagePointers::last_value,
                                              &AdvantagePointers::boot, &AdvantagePointers::advantage, &AdvantagePointers::ret};
    for (auto member : floats) {
        for (uintptr_t off : {4, 8, 12}) {
            AdvantagePointers p = all;
            p.*member += off;
            CHECK(pick_advantage_form(1028, 1028, p).vec == 1, "a float pointer off its 16-byte boundary: V = 1");
        }
        AdvantagePointers p = all;
        p.*member += 16;
        CHECK(pick_advantage_form(1028, 1028, p).vec == 4, "... and on the next one: V = 4");
    }
    for (uintptr_t off : {1, 2, 3}) {
        AdvantagePointers p = all;
        p.done += off;
        CHECK(pick_advantage_form(1028, 1028, p).vec == 1, "the done pointer off its 4-byte boundary: V = 1");
    }
    AdvantagePointers p = all;
    p.done += 4;
    CHECK(pick_advantage_form(1028, 1028, p).vec == 4, "... and on the next one: V = 4");
    // NULL combinations: a NULL pointer constrains nothing and decides has_value / has_boot
    for (int mask = 0; mask < 32; ++mask) {
        p = all;
        if (mask & 1) p.value = 0;
        if (mask & 2) p.boot = 0;
        if (mask & 4) p.last_value = 0;
        if (mask & 8) p.advantage = 0;
        if (mask & 16) p.ret = 0;
        f = pick_advantage_form(1028, 1028, p);
        CHECK(f.vec == 4 && f.has_value == !(mask & 1) && f.has_boot == !(mask & 2), "NULL pointers: still V = 4, the form follows value / boot");
        f = pick_advantage_form(1030, 1030, p);
        CHECK(f.vec == 1 && f.has_value == !(mask & 1) && f.has_boot == !(mask & 2), "... and at V = 1");
    }
    // ... and the threshold itself: below kAdvantageNarrowBelow lanes V = 1 whatever the layout allows, from it on the rules above
    const int64_t edge = gymnet::kAdvantageNarrowBelow;
    CHECK(edge == 4 * 64 * 1024, "one wave of V = 4 threads per SIMD of 1024");
    for (int64_t n : {(int64_t)4, (int64_t)252, (int64_t)1028, edge - 4}) {
        f = gymnet::pick_advantage_form(n, n, all);
        CHECK(f.vec == 1 && f.threads == n && f.blocks == (n + 255) / 256, "below the threshold: V = 1");
    }
    f = gymnet::pick_advantage_form(edge, edge, all);
    CHECK(f.vec == 4 && f.threads == edge / 4 && f.blocks == edge / 1024, "at the threshold: V = 4");
    f = gymnet::pick_advantage_form(edge + 4, edge + 16, all);
    CHECK(f.vec == 4 && f.threads == edge / 4 + 1 && f.blocks == edge / 1024 + 1, "... and a last block that holds one thread");
    CHECK(gymnet::pick_advantage_form(edge + 2, edge + 4, all).vec == 1 && gymnet::pick_advantage_form(edge, edge + 2, all).vec == 1, "the rules still hold above it");
    AdvantagePointers off = all;
    off.advantage += 4;
    CHECK(gymnet::pick_advantage_form(edge, edge, off).vec == 1, "... for pointers too");
}

#ifdef ADVANTAGE_STUB
extern "C" {
typedef struct advantage_stub_call {
    int calls, device;
    void *stream;
    int64_t steps, count, stride;
    float gamma, lambda;
} advantage_stub_call;
const advantage_stub_call *advantage_stub_last(void);
}

static void stub_checks() {
    const int64_t n = 37, T = 5;
    gymnet::VectorEnv env(GYMNET_ENV_CARTPOLE, n, 3);
    const advantage_stub_call *c = advantage_stub_last();
    const Inputs in(T, n);                                       // exactly the documented sizes: the sanitizer sees an access past them
    std::vector<float> adv((size_t)(T * n), -7.0f), ret((size_t)(T * n), -7.0f), want_adv((size_t)(T * n)), want_ret((size_t)(T * n));
    env.AdvantagesDevice(T, in.r.data(), in.d.data(), in.v.data(), in.vlast.data(), adv.data(), ret.data(), 0.75f, 0.5f, in.boot.data());
    CHECK(c->calls == 1 && c->device == 3 && c->stream == nullptr && c->steps == T && c->count == n && c->stride == n, "device, stream and sizes cross");
    CHECK(c->gamma == 0.75f && c->lambda == 0.5f, "gamma and lambda cross");
    recurrence(T, n, in.r.data(), in.d.data(), in.v.data(), in.vlast.data(), in.boot.data(), 0.75f, 0.5f, want_adv.data(), want_ret.data());
    CHECK(same_bits(adv, want_adv) && same_bits(ret, want_ret), "every pointer crosses in its place");
    env.AdvantagesDevice(T, in.r.data(), in.d.data(), in.v.data(), in.vlast.data(), adv.data(), ret.data());
    CHECK(c->calls == 2 && c->gamma == 0.99f && c->lambda == 0.95f, "the defaults: gamma 0.99, lambda 0.95, no boot");
    recurrence(T, n, in.r.data(), in.d.data(), in.v.data(), in.vlast.data(), nullptr, 0.99f, 0.95f, want_adv.data(), want_ret.data());
    CHECK(same_bits(adv, want_adv) && same_bits(ret, want_ret), "... computed without boot");
    // the lean form and a NULL output
    std::fill(ret.begin(), ret.end(), -7.0f);
    env.AdvantagesDevice(T, in.r.data(), in.d.data(), nullptr, nullptr, adv.data(), nullptr, 1.0f, 1.0f);
    recurrence(T, n, in.r.data(), in.d.data(), nullptr, nullptr, nullptr, 1.0f, 1.0f, want_adv.data(), nullptr);
    CHECK(c->calls == 3 && same_bits(adv, want_adv) && ret[0] == -7.0f, "no values, no return");
    // both in-place forms
    recurrence(T, n, in.r.data(), in.d.data(), in.v.data(), in.vlast.data(), in.boot.data(), 0.75f, 0.5f, want_adv.data(), want_ret.data());
    std::vector<float> r2 = in.r, v2 = in.v;
    env.AdvantagesDevice(T, r2.data(), in.d.data(), v2.data(), in.vlast.data(), r2.data(), v2.data(), 0.75f, 0.5f, in.boot.data());
    CHECK(same_bits(r2, want_adv) && same_bits(v2, want_ret), "advantage over reward, return over value");
    r2 = in.r; v2 = in.v;
    env.AdvantagesDevice(T, r2.data(), in.d.data(), v2.data(), in.vlast.data(), v2.data(), r2.data(), 0.75f, 0.5f, in.boot.data());
    CHECK(same_bits(v2, want_adv) && same_bits(r2, want_ret), "advantage over value, return over reward");
    bool refused = false;
    try { env.AdvantagesDevice(T, in.r.data(), in.d.data(), in.v.data(), in.vlast.data(), adv.data(), ret.data(), 1.5f); } catch (const std::exception &) { refused = true; }
    CHECK(refused && c->calls == 5, "a refusal throws");
}
#else
#include <hip/hip_runtime_api.h>

static void cpu_checks() {
    float r[8] = {0}, v[8] = {0}, adv[8], ret[8];
    uint8_t d[8] = {0};
    for (float &x : adv) x = -7.0f;
    for (float &x : ret) x = -7.0f;
    auto call = [&](int64_t steps, int64_t count, int64_t stride, const float *rr, const uint8_t *dd, const float *vv, const float *lv, const float *bb,
                    float g, float l, float *a, float *rt) { return gymnet_gae_device(0, nullptr, steps, count, stride, rr, dd, vv, lv, bb, g, l, a, rt); };
    const float nan = std::nanf(""), inf = INFINITY;
    CHECK(call(-1, 4, 4, r, d, v, v + 4, nullptr, 0.9f, 0.9f, adv, ret) == GYMNET_ERR_INVALID_ARG, "negative steps");
    CHECK(call(1, -1, 4, r, d, v, v + 4, nullptr, 0.9f, 0.9f, adv, ret) == GYMNET_ERR_INVALID_ARG, "negative count");
    CHECK(call(1, 4, 3, r, d, v, v + 4, nullptr, 0.9f, 0.9f, adv, ret) == GYMNET_ERR_INVALID_ARG, "stride < count");
    CHECK(std::string(gymnet_last_error()).find("stride") != std::string::npos, "the message names the stride");
    for (float bad : {-0.1f, 1.5f, nan, inf}) {
        CHECK(call(1, 4, 4, r, d, v, v + 4, nullptr, bad, 0.9f, adv, ret) == GYMNET_ERR_INVALID_ARG, "bad gamma");
        CHECK(std::string(gymnet_last_error()).find("gamma") != std::string::npos, "the message names gamma");
        CHECK(call(1, 4, 4, r, d, v, v + 4, nullptr, 0.9f, bad, adv, ret) == GYMNET_ERR_INVALID_ARG, "bad lambda");
        CHECK(std::string(gymnet_last_error()).find("lambda") != std::string::npos, "the message names lambda");
    }
    CHECK(call(1, 4, 4, nullptr, d, v, v + 4, nullptr, 0.9f, 0.9f, adv, ret) == GYMNET_ERR_INVALID_ARG, "null reward");
    CHECK(call(1, 4, 4, r, nullptr, v, v + 4, nullptr, 0.9f, 0.9f, adv, ret) == GYMNET_ERR_INVALID_ARG, "null done");
    CHECK(call(1, 4, 4, r, d, v, v + 4, nullptr, 0.9f, 0.9f, nullptr, nullptr) == GYMNET_ERR_INVALID_ARG, "both outputs null");
    CHECK(call(1, 4, 4, r, d, v, v + 4, nullptr, 0.9f, 0.9f, adv, adv) == GYMNET_ERR_INVALID_ARG, "advantage == return");
    CHECK(call(1, 4, 4, r, d, v, v + 4, nullptr, 0.9f, 0.9f, reinterpret_cast<float *>(d), ret) == GYMNET_ERR_INVALID_ARG, "an output over done");
    CHECK(call(1, 4, 4, r, d, v, v + 4, ret, 0.9f, 0.9f, adv, ret) == GYMNET_ERR_INVALID_ARG, "an output over boot");
    CHECK(call(1, 4, 4, r, d, v, adv, nullptr, 0.9f, 0.9f, adv, ret) == GYMNET_ERR_INVALID_ARG, "an output over last_value");
    CHECK(std::string(gymnet_last_error()).find("alias") != std::string::npos, "the message says why");
    CHECK(call(0, 4, 4, r, d, v, v + 4, nullptr, 0.9f, 0.9f, adv, ret) == GYMNET_OK, "steps = 0: a no-op");
    CHECK(call(1, 0, 4, r, d, v, v + 4, nullptr, 0.9f, 0.9f, adv, ret) == GYMNET_OK, "count = 0: a no-op");
    bool untouched = true;
    for (float x : adv) untouched &= x == -7.0f;
    for (float x : ret) untouched &= x == -7.0f;
    CHECK(untouched, "nothing written");
    CHECK(GYMNET_ABI_VERSION == 6, "ABI 6");
}

template <class T>
static T *upload(const std::vector<T> &h) {
    T *d = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void **>(&d), sizeof(T) * h.size()) == hipSuccess, "hipMalloc");
    CHECK(hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice) == hipSuccess, "copy");
    return d;
}

static std::vector<float> fetch(const float *d, int64_t count) {
    std::vector<float> out((size_t)count);
    CHECK(hipMemcpy(out.data(), d, sizeof(float) * count, hipMemcpyDeviceToHost) == hipSuccess, "copy");
    return out;
}

static void gpu_checks() {
    const int64_t n = 260, T = 17;
    gymnet::VectorEnv env(GYMNET_ENV_CARTPOLE, n, 0, 7, 0);
    const Inputs in(T, n);
    std::vector<float> want_adv((size_t)(T * n)), want_ret((size_t)(T * n));
    const std::vector<float> poison((size_t)(T * n), -7.25f);
    float *d_r = upload(in.r), *d_v = upload(in.v), *d_vlast = upload(in.vlast), *d_boot = upload(in.boot), *d_adv = upload(poison), *d_ret = upload(poison);
    uint8_t *d_d = upload(in.d);
    env.AdvantagesDevice(T, d_r, d_d, d_v, d_vlast, d_adv, d_ret, 0.99f, 0.95f, d_boot);
    gymnet::check(gymnet_vecenv_sync(env.handle()));
    recurrence(T, n, in.r.data(), in.d.data(), in.v.data(), in.vlast.data(), in.boot.data(), 0.99f, 0.95f, want_adv.data(), want_ret.data());
    CHECK(same_bits(fetch(d_adv, T * n), want_adv) && same_bits(fetch(d_ret, T * n), want_ret), "values, last value and boot: the host recurrence's bits");
    env.AdvantagesDevice(T, d_r, d_d, nullptr, nullptr, d_adv, nullptr, 0.99f, 1.0f);
    gymnet::check(gymnet_vecenv_sync(env.handle()));
    recurrence(T, n, in.r.data(), in.d.data(), nullptr, nullptr, nullptr, 0.99f, 1.0f, want_adv.data(), nullptr);
    CHECK(same_bits(fetch(d_adv, T * n), want_adv) && same_bits(fetch(d_ret, T * n), want_ret), "the lean form; the return array is left alone");
    env.AdvantagesDevice(T, d_r, d_d, d_v, d_vlast, d_r, d_v);                       // in place: advantage over reward, return over value
    gymnet::check(gymnet_vecenv_sync(env.handle()));
    recurrence(T, n, in.r.data(), in.d.data(), in.v.data(), in.vlast.data(), nullptr, 0.99f, 0.95f, want_adv.data(), want_ret.data());
    CHECK(same_bits(fetch(d_r, T * n), want_adv) && same_bits(fetch(d_v, T * n), want_ret), "in place");
    bool refused = false;
    try { env.AdvantagesDevice(T, d_r, d_d, d_v, d_vlast, d_adv, d_adv); } catch (const std::exception &) { refused = true; }
    CHECK(refused, "advantage == return is refused");
    (void)hipFree(d_r); (void)hipFree(d_v); (void)hipFree(d_vlast); (void)hipFree(d_boot); (void)hipFree(d_adv); (void)hipFree(d_ret); (void)hipFree(d_d);
}
#endif

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    picker_checks();
#ifdef ADVANTAGE_STUB
    stub_checks();
    std::printf("stub: %d failed\n", failed);
#else
    cpu_checks();
    if (mode == "--gpu") gpu_checks();
    std::printf("%s: %d failed\n", mode == "--gpu" ? "cpu+gpu" : "cpu", failed);
#endif
    return failed ? 1 : 0;
}
