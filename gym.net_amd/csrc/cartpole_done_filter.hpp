// cartpole_done_filter.hpp — an exact float32 pre-filter for CartPole's done flag.  Plain C++ (no HIP header): the kernels include it
// through envs.hpp, tests/cpp/cartpole_done_filter_test.cpp compiles it with g++.
//
// The flag (envs.hpp CartPole::done_terms_of_inputs) is |v| > T per term, v = RN64(p0 + tau * p1) the binary64 sum of the step's INPUTS
// (position p0, velocity p1; tau * p1 is exact in binary64) and T the float32 threshold widened.  The step also forms the float32 sum
//     P = RN32(tau * p1),   w = RN32(p0 + P)                        (-ffp-contract=off: product, then sum)
// and w decides the flag whenever it is far enough from T.  With e = p0 + tau * p1 (exact):
//     |w - e| <= ulp32(P) / 2 + ulp32(w) / 2,        |P| <= |w| + |p0| + ulp32(w) / 2.
// T lies in a binade [2^k, 2^(k+1)) with u = ulp32(T) = 2^(k-23); both thresholds sit well inside theirs (2.4 in [2, 4), 0.2094 in
// [1/8, 1/4)), and LO = T - 4u, HI = T + 4u are floats of the same binade.
//   NOT DONE.  |p0| < LO and |w| < LO: |P| < 2^(k+2), so ulp32(P) <= 2u and ulp32(w) <= u: |w - e| <= 1.5u, |e| < T - 2.5u, and v, the
//              rounding of e to binary64 (monotone, T is a binary64 value), is below T: the flag is false.
//   DONE.      |p0| < LO and |w| > HI (w may be huge, or infinite): |w - e| <= 2^-24 (|P| + |w|) <= 2^-24 (2|w| + LO) + (tiny), so
//              |e| >= |w| (1 - 2^-23) - 2^-24 LO - (tiny) > T + 4u - (T + 4u) 2^-23 - 2^-24 T > T + 4u - 0.5u - 0.25u > T: the flag is true.
//              (T 2^-23 < 2u 2^-23 2^23 / 2^... : T < 2^(k+1) = 2^24 u, so T 2^-23 < 2u — taken as 2u above would still leave 4u - 2u - u > 0.)
//              An infinite w from finite inputs means |e| >= 2^128 (1 - 2^-25); an infinite p1 gives an infinite v of the same sign.
//   OTHERWISE  AMBIGUOUS — |w| inside [LO, HI], |p0| >= LO, or a NaN anywhere (every compare below is false for a NaN): the caller
//              evaluates the binary64 expression.  The derived error is 1.5u; the band is padded to 4u.
// A subnormal P flushed to zero by the hardware moves w by less than 2^-126: inside the padding.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GYMNET_FILTER_HD __host__ __device__ __forceinline__
#else
#define GYMNET_FILTER_HD inline
#endif

namespace gymnet {

struct CartPoleDoneBand {
    // float32 ulp at each threshold: 2.4 = 0x1.333334p+1 -> 2^-22; 0.20943952 = 0x1.aceeap-3 -> 2^-26
    static constexpr float x_threshold = 2.4f, x_ulp = 0x1p-22f;
    static constexpr float theta_threshold = 0.20943951606750488f, theta_ulp = 0x1p-26f;
    static constexpr float x_lo = x_threshold - 4.0f * x_ulp, x_hi = x_threshold + 4.0f * x_ulp;                      // exact: same binade
    static constexpr float theta_lo = theta_threshold - 4.0f * theta_ulp, theta_hi = theta_threshold + 4.0f * theta_ulp;
};

// One term.  `done` is the flag where the return value (decided) is true; where it is false the caller must not use `done`.
//   p0  the position the step started with        w  the float32 sum RN32(p0 + RN32(tau * p1))
// (the three compares on their own: a kernel takes each one's wave mask and combines the masks on the scalar unit)
GYMNET_FILTER_HD void cartpole_done_compares(float p0, float w, float lo, float hi, bool &inside, bool &below, bool &above) {
    const float a0 = __builtin_fabsf(p0), aw = __builtin_fabsf(w);
    inside = a0 < lo;
    below = aw < lo;
    above = aw > hi;
}
GYMNET_FILTER_HD bool cartpole_done_term_f32(float p0, float w, float lo, float hi, bool &done) {
    bool inside, below;
    cartpole_done_compares(p0, w, lo, hi, inside, below, done);
    return inside && (below || done);
}

}  // namespace gymnet
