// episode_memory_key.hpp — the order of the episode memory's keys.  Plain C++ (no HIP header): episode_memory.hip includes it for the
// kernels and for the host sort of gymnet_vecenv_memory_episodes, tests/cpp/episode_memory_key_test.cpp compiles it with g++.
//
// A kept episode's key is (return, end tick, lane), ordered lexicographically.  The return goes in as ret_bits, an unsigned integer that
// orders like the float: +0 and -0 are one value, +-inf and denormals are ordinary values.  A NaN has no place in that order (ret_bits
// would put a positive one above +inf and a negative one below -inf), so the admission predicate keeps every NaN out of the pool:
// the pool, the threshold and the host sort never see one.  Equal keys can exist (a tick set backwards, or a replay after a restored
// checkpoint): key_less is then false both ways, the kept set is the top-K MULTISET of keys, and whoever ranks or selects breaks the
// tie by pool position (episode_memory.hip: merge_body, memory_rank_kernel).
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GYMNET_KEY_HD __host__ __device__ __forceinline__
#else
#define GYMNET_KEY_HD inline
#endif

namespace gymnet {

// a float's order as an unsigned integer (+0 and -0 are one value)
GYMNET_KEY_HD uint32_t ret_bits(float r) {
    const uint32_t u = __builtin_bit_cast(uint32_t, r == 0.0f ? 0.0f : r);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
GYMNET_KEY_HD float bits_ret(uint32_t b) { return __builtin_bit_cast(float, (b & 0x80000000u) ? (b ^ 0x80000000u) : ~b); }

struct Key { uint32_t w[4]; };      // (return, tick high, tick low, lane): 16 digits of 8 bits, most significant first

GYMNET_KEY_HD Key make_key(float ret, uint64_t tick, int32_t lane) {
    Key k;
    k.w[0] = ret_bits(ret); k.w[1] = (uint32_t)(tick >> 32); k.w[2] = (uint32_t)tick; k.w[3] = (uint32_t)lane;
    return k;
}

GYMNET_KEY_HD bool key_less(const Key &a, const Key &b) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (a.w[q] != b.w[q]) return a.w[q] < b.w[q];
    return false;
}

// the order gymnet_vecenv_memory_episodes lists the pool in: descending key (a strict weak order: the keys are integers)
GYMNET_KEY_HD bool key_before(const Key &a, const Key &b) { return key_less(b, a); }

// the dataset's order of pool entries ia and ib: descending key, equal keys by pool index — every entry gets a rank of its own
GYMNET_KEY_HD bool key_ranks_before(const Key &a, int ia, const Key &b, int ib) {
    return key_less(b, a) || (!key_less(a, b) && ia < ib);
}

GYMNET_KEY_HD uint32_t digit(const Key &k, int d) {
    uint32_t w = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) if (q == (d >> 2)) w = k.w[q];
    return (w >> (24 - 8 * (d & 3))) & 255u;
}

// digits 0 .. d-1 of k equal those of t
GYMNET_KEY_HD bool prefix_match(const Key &k, const uint32_t (&t)[4], int d) {
    const int wd = d >> 2, b = d & 3;
    const uint32_t mask = b ? 0xFFFFFFFFu << (32 - 8 * b) : 0u;
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q < wd) ok &= k.w[q] == t[q];
        else if (q == wd) ok &= (k.w[q] & mask) == (t[q] & mask);
    }
    return ok;
}

// An ended episode goes on to the merge: it is not too long, its return is a number, and the pool has room or its return is at least
// the lowest kept one (a newer episode wins ties of return).  full / thr: the pool's state as the caller read it.
GYMNET_KEY_HD bool memory_admits(bool too_long, bool full, float ret, float thr) {
    return !too_long && ret == ret && (!full || ret >= thr);
}

}  // namespace gymnet
