// log_pos.hpp — ln(x) for a normal positive float32, operation for operation, so that a CPU reproduces its bits (HIP == twin
// bitwise; the device library's logf and v_log_f32 cannot be restated on a host).  The log-probability a Discrete actor records
// (actor_logp.hip) is its one user: L = log_pos(S) of the softmax's sum S in [1, 8]; tests/_actor_logp_twin.py restates it in C with the
// same constants.  Compiled with -ffp-contract=off: every operation below rounds on its own, the multiply-adds are explicit fmaf.
//   i = bits(x) + (bits(1.0f) - bits(sqrt(0.5)))   integer: the exponent field steps where the mantissa passes sqrt(2)
//   k = (i >> 23) - 127                            x = m * 2^k with m in [sqrt(0.5), sqrt(2))
//   m = float((i & 0x007fffff) + bits(sqrt(0.5)))  the same mantissa under the exponent of that range
//   f = m - 1                                      exact; f in [-0.293, 0.414]
//   z = f * f
//   p = P(f)                                       degree 8 (the Cephes logf coefficients, ln(1 + f) = f - f^2 / 2 + f^3 * P(f)), Horner, fmaf
//   r = fmaf(-0.5, z, (f * z) * p)                 everything of ln(m) but f itself; |r| < 0.09
//   hi = k * kLogPosLn2Hi                          exact: ln2_hi has 9 significant bits
//   s = hi + f,  c = f - (s - hi)                  s + c = hi + f exactly (|hi| >= |f| where k != 0; k = 0 gives s = f, c = 0)
//   result = s + ((fmaf(k, kLogPosLn2Lo, r)) + c)
// The large terms (hi, f) are summed without error and the last addition rounds once, so what reaches it is off by far less than the
// step of ln between neighbouring arguments.  Over every float32 in [1, 8] (tests/test_actor_logp_host.py): log_pos(1.0f) is +0.0f, no
// result is below +0, the function is non-decreasing, and the absolute error against float64 log is at most 1.20e-7 (measured; half a
// spacing of float32 at ln 8).
#pragma once
#include <stdint.h>

namespace gymnet {

constexpr int32_t kLogPosSqrtHalfBits = 0x3f3504f3, kLogPosOneBits = 0x3f800000;
constexpr float kLogPosLn2Hi = 0.693359375f, kLogPosLn2Lo = -2.12194440e-4f;
constexpr float kLogPosP0 = 7.0376836292e-2f, kLogPosP1 = -1.1514610310e-1f, kLogPosP2 = 1.1676998740e-1f, kLogPosP3 = -1.2420140846e-1f,
                kLogPosP4 = 1.4249322787e-1f, kLogPosP5 = -1.6668057665e-1f, kLogPosP6 = 2.0000714765e-1f, kLogPosP7 = -2.4999993993e-1f,
                kLogPosP8 = 3.3333331174e-1f;

__host__ __device__ __forceinline__ float log_pos(float x) {
    int32_t i = __builtin_bit_cast(int32_t, x) + (kLogPosOneBits - kLogPosSqrtHalfBits);
    const float k = (float)((i >> 23) - 127);
    i = (i & 0x007fffff) + kLogPosSqrtHalfBits;
    const float f = __builtin_bit_cast(float, i) - 1.0f;
    const float z = f * f;
    float p = kLogPosP0;
    p = __builtin_fmaf(p, f, kLogPosP1);
    p = __builtin_fmaf(p, f, kLogPosP2);
    p = __builtin_fmaf(p, f, kLogPosP3);
    p = __builtin_fmaf(p, f, kLogPosP4);
    p = __builtin_fmaf(p, f, kLogPosP5);
    p = __builtin_fmaf(p, f, kLogPosP6);
    p = __builtin_fmaf(p, f, kLogPosP7);
    p = __builtin_fmaf(p, f, kLogPosP8);
    const float y = (f * z) * p;
    const float r = __builtin_fmaf(-0.5f, z, y);
    const float hi = k * kLogPosLn2Hi;
    const float s = hi + f;
    const float c = f - (s - hi);
    const float t = __builtin_fmaf(k, kLogPosLn2Lo, r) + c;
    return s + t;
}

}  // namespace gymnet
