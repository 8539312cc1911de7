// cartpole_done_filter_test.cpp — gym.net_amd/csrc/cartpole_done_filter.hpp on the CPU (g++ -std=c++17 -ffp-contract=off; no HIP).
//   (no argument)  the sweeps below: wherever the filter decides a term, its flag must be the binary64 expression's
//   eval           stdin: one "x x_dot theta theta_dot" per line as float32 bit patterns in hex; stdout per line
//                  "decided_x flag_x exact_x decided_theta flag_theta exact_theta"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "cartpole_done_filter.hpp"

using gymnet::CartPoleDoneBand;

static const float kTau = 0.02f;

static float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
static uint32_t to_bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
// d float32 steps away from a finite non-zero f, away from zero for d > 0
static float steps(float f, int d) { return from_bits(to_bits(f) + (uint32_t)d); }

// what the step forms in float32 (product, then sum: two roundings) ...
static float sum_f32(float p0, float p1) { volatile float P = kTau * p1; volatile float w = p0 + P; return w; }
// ... and what the reference compares (CartPole::done_terms_of_inputs)
static bool exact(float p0, float p1, float thr) { return std::fabs(std::fma((double)kTau, (double)p1, (double)p0)) > (double)thr; }

struct Tally { long total = 0, decided = 0, wrong = 0; };

static void check(float p0, float p1, float thr, float lo, float hi, Tally &t) {
    bool done = false;
    const bool decided = gymnet::cartpole_done_term_f32(p0, sum_f32(p0, p1), lo, hi, done);
    ++t.total;
    if (!decided) return;
    ++t.decided;
    if (done != exact(p0, p1, thr)) {
        ++t.wrong;
        if (t.wrong <= 10) std::printf("WRONG p0=%a p1=%a thr=%a: filter %d, exact %d\n", p0, p1, thr, (int)done, (int)exact(p0, p1, thr));
    }
}

static int sweep(const char *name, float thr, float lo, float hi) {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float tiny = std::numeric_limits<float>::denorm_min(), small = std::numeric_limits<float>::min(), big = 1e30f, huge = std::numeric_limits<float>::max();
    std::vector<float> vel = {0.0f, -0.0f, tiny, -tiny, small, -small, 1e-7f, -1e-7f, 1e-3f, -1e-3f, 0.5f, -0.5f, 3.0f, -3.0f, 250.0f, -250.0f,
                              big, -big, huge, -huge, nan, inf, -inf};
    Tally a, b, c;
    // 1. every position within 64 steps of +-threshold, the whole velocity grid, and velocities that bring the sum back inside
    for (int sign = -1; sign <= 1; sign += 2)
        for (int d = -64; d <= 64; ++d) {
            const float p0 = (float)sign * steps(thr, d);
            for (float v : vel) check(p0, v, thr, lo, hi, a);
            for (int e = -8; e <= 8; ++e) check(p0, (float)(-sign) * steps(thr * 50.0f, e), thr, lo, hi, a);       // sum near zero
            for (int e = -8; e <= 8; ++e) check(p0, (float)(-sign) * steps(thr * 100.0f, e), thr, lo, hi, a);      // sum near the other threshold
        }
    // 2. positions well inside (and NaN / infinite / far outside), velocities that put the SUM within 64 steps of +-threshold
    const float starts[] = {0.0f, thr * 0.01f, thr * 0.25f, thr * 0.5f, thr * 0.9f, steps(lo, -1), lo, -thr * 0.01f, -thr * 0.25f, -thr * 0.5f, -thr * 0.9f,
                            -steps(lo, -1), -lo, thr * 4.0f, -thr * 4.0f, 1e30f, nan, inf, -inf};
    for (float p0 : starts)
        for (int sign = -1; sign <= 1; sign += 2)
            for (int d = -64; d <= 64; ++d) {
                const double target = (double)((float)sign * steps(thr, d));
                const float v0 = (float)((target - (double)p0) / (double)kTau);
                if (!(std::fabs(v0) > 0.0f) || std::isinf(v0)) { check(p0, v0, thr, lo, hi, b); continue; }
                for (int e = -6; e <= 6; ++e) check(p0, steps(v0, e), thr, lo, hi, b);
            }
    // 3. the grid against itself
    for (float p0 : vel)
        for (float v : vel) check(p0, v, thr, lo, hi, c);
    std::printf("%s: near-threshold positions %ld cases, %ld decided, %ld wrong; near-threshold sums %ld cases, %ld decided, %ld wrong; grid %ld cases, %ld decided, %ld wrong\n",
                name, a.total, a.decided, a.wrong, b.total, b.decided, b.wrong, c.total, c.decided, c.wrong);
    // the filter is of use only if it decides what is not close: some of each sweep, and not everything of the first two
    const bool useful = a.decided > 0 && a.decided < a.total && b.decided > 0 && b.decided < b.total && c.decided > 0;
    if (!useful) std::printf("%s: the filter decides nothing or everything\n", name);
    return (a.wrong + b.wrong + c.wrong == 0 && useful) ? 0 : 1;
}

int main(int argc, char **argv) {
    typedef CartPoleDoneBand B;
    if (argc > 1 && std::strcmp(argv[1], "eval") == 0) {
        unsigned x, xd, th, thd;
        while (std::scanf("%x %x %x %x", &x, &xd, &th, &thd) == 4) {
            const float p[4] = {from_bits(x), from_bits(xd), from_bits(th), from_bits(thd)};
            bool fx = false, ft = false;
            const bool dx = gymnet::cartpole_done_term_f32(p[0], sum_f32(p[0], p[1]), B::x_lo, B::x_hi, fx);
            const bool dt = gymnet::cartpole_done_term_f32(p[2], sum_f32(p[2], p[3]), B::theta_lo, B::theta_hi, ft);
            std::printf("%d %d %d %d %d %d\n", (int)dx, (int)fx, (int)exact(p[0], p[1], B::x_threshold), (int)dt, (int)ft, (int)exact(p[2], p[3], B::theta_threshold));
        }
        return 0;
    }
    // the band is four float32 steps either side of each threshold, in the threshold's binade
    int bad = 0;
    bad += !(to_bits(B::x_threshold) - to_bits(B::x_lo) == 4 && to_bits(B::x_hi) - to_bits(B::x_threshold) == 4);
    bad += !(to_bits(B::theta_threshold) - to_bits(B::theta_lo) == 4 && to_bits(B::theta_hi) - to_bits(B::theta_threshold) == 4);
    if (bad) std::printf("the band's constants are not threshold -+ 4 ulps\n");
    bad += sweep("x", B::x_threshold, B::x_lo, B::x_hi);
    bad += sweep("theta", B::theta_threshold, B::theta_lo, B::theta_hi);
    std::printf(bad ? "FAILED\n" : "filter never decides wrongly\n");
    return bad ? 1 : 0;
}
