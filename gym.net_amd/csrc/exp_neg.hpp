// exp_neg.hpp — exp(a) for a <= 0 in float32, operation for operation, so that a CPU reproduces its bits (HIP == twin bitwise;
// the device library's expf and v_exp_f32 cannot be restated on a host).  The softmax draw of a Discrete actor (actor_softmax.hip) is its
// one user; tests/_actor_softmax_twin.py restates it in C with the same constants.  Compiled with -ffp-contract=off: every operation below
// rounds on its own, the multiply-adds are explicit fmaf.
//   t = a * log2(e)                      one product
//   t >= -125 fails (also a NaN)         -> +0.0f: the weight has underflowed, the action cannot be drawn
//   n = rintf(t), f = t - n              round to nearest even; f in [-0.5, 0.5], exact
//   p = 2^f                              degree-7 Taylor polynomial in f (coefficients ln2^k / k!, rounded to float32), Horner, fmaf
//   result = p with n added to its exponent field as integer bits (p in [0.70, 1.42], n in [-125, 0]: the result stays normal)
// Over every float32 in [-104, 0] the absolute error against float64 exp is at most 5.5e-8 (tests/test_actor_softmax_host.py measures it).
#pragma once
#include <stdint.h>

namespace gymnet {

constexpr float kExpNegLog2e = 1.44269504088896341f;
constexpr float kExpNegC1 = 0.693147180559945309f, kExpNegC2 = 0.240226506959100712f, kExpNegC3 = 0.0555041086648215800f,
                kExpNegC4 = 0.00961812910762847716f, kExpNegC5 = 0.00133335581464284434f, kExpNegC6 = 0.000154035303933816099f,
                kExpNegC7 = 0.0000152527338040598403f;

__host__ __device__ __forceinline__ float exp_neg(float a) {
    const float t = a * kExpNegLog2e;
    if (!(t >= -125.0f)) return 0.0f;
    const float n = __builtin_rintf(t);
    const float f = t - n;
    float p = kExpNegC7;
    p = __builtin_fmaf(p, f, kExpNegC6);
    p = __builtin_fmaf(p, f, kExpNegC5);
    p = __builtin_fmaf(p, f, kExpNegC4);
    p = __builtin_fmaf(p, f, kExpNegC3);
    p = __builtin_fmaf(p, f, kExpNegC2);
    p = __builtin_fmaf(p, f, kExpNegC1);
    p = __builtin_fmaf(p, f, 1.0f);
    const int32_t bits = __builtin_bit_cast(int32_t, p) + (int32_t)n * (1 << 23);
    return __builtin_bit_cast(float, bits);
}

}  // namespace gymnet
