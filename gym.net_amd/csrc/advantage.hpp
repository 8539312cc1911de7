// advantage.hpp — which form of the advantage kernel (advantage.hip) a call to gymnet_gae_device launches.  Host-only and pure: no HIP
// type, no global, nothing read but the arguments, so tests/cpp/advantage_test.cpp runs it as a stand-alone program.  This is the only
// place that picks the form.
//
// One thread owns V consecutive lanes (columns) and walks the rows t = T-1 .. 0.  V = 4 moves 16 bytes per access of reward / value /
// boot / advantage / return and the four done bytes as one 4-byte word; it needs every row of every array to start a 16-byte (done: 4-byte)
// unit at the thread's first column, which holds exactly when
//     count % 4 == 0,  stride % 4 == 0,  every non-NULL float pointer is 16-byte aligned,  the done pointer is 4-byte aligned.
// Anything else runs V = 1, and so does any count below kAdvantageNarrowBelow.  Whether values and boot exist is part of the form (a template parameter of the kernel: the lean forms
// read nothing they do not need); whether an output is NULL is not (a wave-uniform branch in the kernel).
#pragma once
#include <cstdint>

namespace gymnet {

struct AdvantagePointers {                        // the call's pointers as integers; 0 = NULL
    uintptr_t reward, done, value, last_value, boot, advantage, ret;
};

struct AdvantageForm {
    int vec;                                      // lanes per thread: 1 or 4
    bool has_value, has_boot;
    int64_t threads;                              // count / vec, rounded up: one thread per vec lanes
    int64_t blocks;                               // of 256 threads
};

constexpr int kAdvantageBlock = 256;
// Lane counts below this run V = 1 for four times the waves.  4 lanes x 64 threads x 1024 SIMDs of an MI355X: below it V = 4 cannot give
// every SIMD a wave.  Measured (docs/ledger.md §advantage): V = 1 is 1.3 to 2 times faster up to 2^16 lanes, V = 4 1.3 times faster from 2^18.
constexpr int64_t kAdvantageNarrowBelow = 4 * 64 * 1024;

inline AdvantageForm pick_advantage_form(int64_t count, int64_t stride, const AdvantagePointers &p, int64_t narrow_below = kAdvantageNarrowBelow) {
    const uintptr_t floats = p.reward | p.value | p.last_value | p.boot | p.advantage | p.ret;      // (NULL contributes no bit)
    const bool wide = count >= narrow_below && count % 4 == 0 && stride % 4 == 0 && (floats & 15u) == 0 && (p.done & 3u) == 0;
    AdvantageForm f;
    f.vec = wide ? 4 : 1;
    f.has_value = p.value != 0;
    f.has_boot = p.boot != 0;
    f.threads = (count + f.vec - 1) / f.vec;
    f.blocks = (f.threads + kAdvantageBlock - 1) / kAdvantageBlock;
    return f;
}

}  // namespace gymnet
