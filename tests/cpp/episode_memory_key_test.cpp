// episode_memory_key_test.cpp — gym.net_amd/csrc/episode_memory_key.hpp on the CPU (g++ -std=c++17; no HIP, no library).
//   (no argument)  the header's functions against plain restatements: ret_bits against the float order, key_less against the
//                  lexicographic order of (return, tick, lane), the 16-pass digit selection against a sort, the admission predicate
//                  against NaN, the listing order's strict-weak-order axioms, the rank rule and the merge rule with equal keys.
//                  Prints "key: <checks> checks, <n> failed".
//   --before       the same checks of predicate, listing order, rank rule and merge rule against the rules as they were before NaN and
//                  equal keys were specified (restated below): prints how many rows each of them fails, "before: <name> <n> failed".
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <tuple>
#include <vector>

#include "../../gym.net_amd/csrc/episode_memory_key.hpp"

using gymnet::Key;

static float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
static uint32_t to_bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

static long g_checks = 0, g_failed = 0;
static void expect(bool ok, const char *what, uint64_t a = 0, uint64_t b = 0) {
    ++g_checks;
    if (ok) return;
    if (++g_failed <= 20) std::printf("FAILED %s (%llx, %llx)\n", what, (unsigned long long)a, (unsigned long long)b);
}

struct Ep { float ret; uint64_t tick; int32_t lane; };
static Key key_of(const Ep &e) { return gymnet::make_key(e.ret, e.tick, e.lane); }
// the order the contract states, in plain terms: the float order (+0 == -0), then the tick, then the lane
static bool plain_less(const Ep &a, const Ep &b) {
    if (a.ret != b.ret) return a.ret < b.ret;
    return std::make_tuple(a.tick, a.lane) < std::make_tuple(b.tick, b.lane);
}

// ---- 1. ret_bits ----------------------------------------------------------------------------------------------------------------------
static std::vector<float> edge_floats() {
    const uint32_t anchors[] = {0x00000000u, 0x00800000u, 0x3F800000u, 0x7F7FFFFFu, 0x7F800000u};      // 0, FLT_MIN, 1, FLT_MAX, inf
    std::vector<float> v;
    for (uint32_t sign : {0u, 0x80000000u})
        for (uint32_t a : anchors)
            for (int d = -64; d <= 64; ++d) {
                const int64_t m = (int64_t)a + d;
                if (m < 0 || m > 0x7F800000) continue;                  // below zero's pattern, or a NaN
                v.push_back(from_bits(sign | (uint32_t)m));
            }
    return v;
}

static void test_ret_bits() {
    std::vector<float> v = edge_floats();
    const size_t edges = v.size();
    for (size_t i = 0; i < edges; ++i)                                  // every pair of the edge values
        for (size_t j = 0; j < edges; ++j) {
            const uint32_t bi = gymnet::ret_bits(v[i]), bj = gymnet::ret_bits(v[j]);
            expect((v[i] < v[j]) == (bi < bj) && (v[i] == v[j]) == (bi == bj), "ret_bits order (edges)", to_bits(v[i]), to_bits(v[j]));
        }
    std::mt19937 rng(20240607u);
    for (int i = 0; i < (1 << 20); ++i) {
        const float f = from_bits((uint32_t)rng());
        if (f == f) v.push_back(f);
    }
    std::sort(v.begin(), v.end());
    for (size_t i = 0; i + 1 < v.size(); ++i) {
        const uint32_t a = gymnet::ret_bits(v[i]), b = gymnet::ret_bits(v[i + 1]);
        expect(v[i] < v[i + 1] ? a < b : a == b, "ret_bits monotone (sweep)", to_bits(v[i]), to_bits(v[i + 1]));
    }
    for (float f : v) {
        const float back = gymnet::bits_ret(gymnet::ret_bits(f));
        expect(back == f && (f == 0.0f || to_bits(back) == to_bits(f)), "bits_ret(ret_bits(x)) == x", to_bits(f), to_bits(back));
    }
    expect(gymnet::ret_bits(-0.0f) == gymnet::ret_bits(0.0f), "ret_bits(-0) == ret_bits(+0)");
}

// ---- 2. key_less on keys that differ in one digit -------------------------------------------------------------------------------------
// the episode whose key words are w, or false when no episode has them (the return word is a NaN's, or -0's)
static bool ep_of_words(const uint32_t (&w)[4], Ep *e) {
    const float r = gymnet::bits_ret(w[0]);
    if (!(r == r) || gymnet::ret_bits(r) != w[0] || (w[3] & 0x80000000u)) return false;
    *e = Ep{r, ((uint64_t)w[1] << 32) | w[2], (int32_t)w[3]};
    return true;
}

static void check_pair(const Ep &a, const Ep &b, const char *what) {
    expect(gymnet::key_less(key_of(a), key_of(b)) == plain_less(a, b), what, to_bits(a.ret), to_bits(b.ret));
    expect(gymnet::key_less(key_of(b), key_of(a)) == plain_less(b, a), what, to_bits(b.ret), to_bits(a.ret));
}

static void test_key_less() {
    std::mt19937 rng(77u);
    int per_digit[16] = {};
    for (int trial = 0; trial < 4000; ++trial) {
        uint32_t w[4] = {(uint32_t)rng(), (uint32_t)rng(), (uint32_t)rng(), (uint32_t)rng() & 0x7FFFFFFFu};
        if (trial % 4 == 0) w[1] = 0u;                                   // ticks below 2^32 too
        Ep a;
        if (!ep_of_words(w, &a)) continue;
        for (int d = 0; d < 16; ++d) {
            const int sh = 24 - 8 * (d & 3);
            const uint32_t old = (w[d >> 2] >> sh) & 255u;
            for (uint32_t nv : {(old + 1u) & 255u, (uint32_t)rng() & 255u, 0u, 255u}) {
                if (nv == old) continue;
                uint32_t x[4] = {w[0], w[1], w[2], w[3]};
                x[d >> 2] = (x[d >> 2] & ~(255u << sh)) | (nv << sh);
                Ep b;
                if (!ep_of_words(x, &b)) continue;
                check_pair(a, b, "key_less, one digit differs");
                expect(gymnet::digit(key_of(a), d) == old && gymnet::digit(key_of(b), d) == nv, "digit", (uint64_t)d);
                ++per_digit[d];
            }
            // a carry: ..FF in this digit and below against the next value, ..00
            uint32_t lo[4] = {w[0], w[1], w[2], w[3]}, hi[4];
            for (int q = d; q < 16; ++q) lo[q >> 2] |= 255u << (24 - 8 * (q & 3));
            std::memcpy(hi, lo, sizeof hi);
            for (int q = 3; q >= 0; --q) if (++hi[q] != 0u) break;
            Ep l, h;
            if (ep_of_words(lo, &l) && ep_of_words(hi, &h)) check_pair(l, h, "key_less, carry");
        }
    }
    for (int d = 0; d < 16; ++d) expect(per_digit[d] > 1000, "every digit got its pairs", (uint64_t)d);
}

// ---- 3. the digit selection -----------------------------------------------------------------------------------------------------------
// merge_body's selection, restated for one thread: the cap-th largest of keys (cap <= keys.size())
static Key select_kth(const std::vector<Key> &keys, uint32_t cap) {
    uint32_t tau[4] = {0u, 0u, 0u, 0u}, need = cap;
    for (int d = 0; d < 16; ++d) {
        uint32_t hist[256] = {};
        const uint32_t t[4] = {tau[0], tau[1], tau[2], tau[3]};
        for (const Key &k : keys)
            if (gymnet::prefix_match(k, t, d)) ++hist[gymnet::digit(k, d)];
        uint32_t cum = 0u;
        int b = 255;
        for (; b > 0; --b) {
            if (cum + hist[b] >= need) break;
            cum += hist[b];
        }
        need -= cum;
        tau[d >> 2] |= (uint32_t)b << (24 - 8 * (d & 3));
    }
    Key k;
    for (int q = 0; q < 4; ++q) k.w[q] = tau[q];
    return k;
}

static bool same_key(const Key &a, const Key &b) { return !gymnet::key_less(a, b) && !gymnet::key_less(b, a); }

static void check_selection(std::vector<Key> keys, const char *what) {
    std::vector<Key> sorted = keys;
    std::sort(sorted.begin(), sorted.end(), [](const Key &a, const Key &b) { return gymnet::key_before(a, b); });
    for (uint32_t cap = 1; cap <= keys.size(); cap += (keys.size() > 64 ? 37 : 1))
        expect(same_key(select_kth(keys, cap), sorted[cap - 1]), what, cap, keys.size());
    expect(same_key(select_kth(keys, (uint32_t)keys.size()), sorted.back()), what, keys.size(), keys.size());
}

static void test_selection() {
    std::mt19937 rng(4242u);
    for (int set = 0; set < 40; ++set) {                                 // random keys, then the same with duplicates
        std::vector<Key> keys;
        const int count = 1 + (int)(rng() % 600);
        for (int i = 0; i < count; ++i) {
            uint32_t w[4] = {(uint32_t)rng(), (uint32_t)rng() & (set & 1 ? 0xFFFFFFFFu : 1u), (uint32_t)rng(), (uint32_t)rng() & 0xFFFFFu};
            Ep e;
            if (ep_of_words(w, &e)) keys.push_back(key_of(e));
        }
        if (keys.empty()) continue;
        check_selection(keys, "selection, random keys");
        for (int i = 0; i < count / 3; ++i) keys.push_back(keys[rng() % keys.size()]);
        check_selection(keys, "selection, random keys with duplicates");
    }
    for (int d = 0; d < 16; ++d) {                                       // keys that differ in digit d alone, every value of it, some twice
        std::vector<Key> keys;
        const uint32_t base[4] = {0xC0490FDBu, 0x00000001u, 0xFFFFFF00u, 0x0000FFFFu};
        for (uint32_t v = 0; v < 256; ++v) {
            uint32_t x[4] = {base[0], base[1], base[2], base[3]};
            const int sh = 24 - 8 * (d & 3);
            x[d >> 2] = (x[d >> 2] & ~(255u << sh)) | (v << sh);
            Ep e;
            if (!ep_of_words(x, &e)) continue;
            keys.push_back(key_of(e));
            if (v % 5 == 0) keys.push_back(key_of(e));
        }
        check_selection(keys, "selection, one digit differs");
    }
    std::vector<Key> one(300, key_of(Ep{1.5f, 7ull, 3}));                 // every key equal
    check_selection(one, "selection, all keys equal");
    std::vector<Key> edge;                                               // the returns at the sign fold, each twice
    for (float f : edge_floats()) { edge.push_back(key_of(Ep{f, 9ull, 1})); edge.push_back(key_of(Ep{f, 9ull, 1})); }
    check_selection(edge, "selection, sign fold");
}

// ---- 4. the admission predicate -------------------------------------------------------------------------------------------------------
using Admits = bool (*)(bool, bool, float, float);
static bool admits_before(bool too_long, bool full, float ret, float thr) { return !too_long && (!full || ret >= thr); }

static void test_admission(Admits admits) {
    const float inf = std::numeric_limits<float>::infinity();
    const uint32_t nans[] = {0x7FC00000u, 0xFFC00000u, 0x7FC00001u, 0xFFC12345u, 0x7F800001u, 0xFF800001u, 0x7FFFFFFFu, 0xFFFFFFFFu};
    const float thrs[] = {-inf, -1.0f, -0.0f, 0.0f, 1e-45f, 1.0f, 3.4e38f, inf};
    for (uint32_t nb : nans)
        for (float thr : thrs)
            for (int full = 0; full < 2; ++full) expect(!admits(false, full != 0, from_bits(nb), thr), "a NaN return is refused", nb, (uint64_t)full);
    for (float ret : thrs) {
        expect(admits(false, false, ret, 123.0f), "a pool with room admits every number", to_bits(ret));
        expect(!admits(true, false, ret, 123.0f) && !admits(true, true, ret, ret), "too long is refused", to_bits(ret));
        for (float thr : thrs) expect(admits(false, true, ret, thr) == (ret >= thr), "a full pool admits ret >= thr", to_bits(ret), to_bits(thr));
    }
    expect(admits(false, true, -0.0f, 0.0f) && admits(false, true, 0.0f, -0.0f), "the zeros tie");
}

// ---- 5. the listing order -------------------------------------------------------------------------------------------------------------
using Before = bool (*)(const Ep &, const Ep &);
static bool before_now(const Ep &a, const Ep &b) { return gymnet::key_before(key_of(a), key_of(b)); }
static bool before_before(const Ep &a, const Ep &b) {                    // the lambda gymnet_vecenv_memory_episodes sorted with
    auto ret_order = [](float r) { return r == 0.0f ? 0.0f : r; };
    if (ret_order(a.ret) != ret_order(b.ret)) return ret_order(a.ret) > ret_order(b.ret);
    if (a.tick != b.tick) return a.tick > b.tick;
    return a.lane > b.lane;
}

static void test_strict_weak_order(Before before, bool with_nan) {
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<Ep> v;
    for (float r : {0.0f, -0.0f, 1e-45f, -1e-45f, 1.17549435e-38f, -1.17549435e-38f, 1.0f, -1.0f, inf, -inf, 3.4028235e38f})
        for (uint64_t tick : {5ull, (1ull << 32) + 5ull})
            for (int32_t lane : {0, 256}) v.push_back(Ep{r, tick, lane});
    v.push_back(v[3]); v.push_back(v[17]); v.push_back(v[17]);            // equal keys
    if (with_nan) { v.push_back(Ep{from_bits(0x7FC00000u), 5ull, 1}); v.push_back(Ep{from_bits(0xFFC00000u), 6ull, 2}); }
    const size_t n = v.size();
    auto equiv = [&](size_t i, size_t j) { return !before(v[i], v[j]) && !before(v[j], v[i]); };
    for (size_t i = 0; i < n; ++i) {
        expect(!before(v[i], v[i]), "irreflexive", i);
        for (size_t j = 0; j < n; ++j) {
            expect(!(before(v[i], v[j]) && before(v[j], v[i])), "asymmetric", i, j);
            for (size_t k = 0; k < n; ++k) {
                expect(!(before(v[i], v[j]) && before(v[j], v[k])) || before(v[i], v[k]), "transitive", i, k);
                expect(!(equiv(i, j) && equiv(j, k)) || equiv(i, k), "equivalence is transitive", i, k);
            }
        }
    }
    if (!with_nan) {                                                     // and std::sort with it, under the sanitizers
        std::mt19937 rng(5u);
        std::shuffle(v.begin(), v.end(), rng);
        std::sort(v.begin(), v.end(), before);
        for (size_t i = 0; i + 1 < n; ++i) expect(!plain_less(v[i], v[i + 1]), "sorted descending", i);
    }
}

// ---- 6. the rank rule and the merge rule with equal keys ------------------------------------------------------------------------------
// memory_rank_kernel: the dataset position of pool entry i
using Rank = int (*)(const std::vector<Key> &, int);
static int rank_now(const std::vector<Key> &pool, int i) {
    int r = 0;
    for (int j = 0; j < (int)pool.size(); ++j) r += gymnet::key_ranks_before(pool[j], j, pool[i], i) ? 1 : 0;
    return r;
}
static int rank_before(const std::vector<Key> &pool, int i) {
    int r = 0;
    for (int j = 0; j < (int)pool.size(); ++j) r += gymnet::key_less(pool[i], pool[j]) ? 1 : 0;
    return r;
}

static void test_rank(Rank rank) {
    std::vector<Key> pool;
    for (int i = 0; i < 40; ++i) pool.push_back(key_of(Ep{(float)(i % 7), (uint64_t)(i % 3), 0}));      // 40 entries of 21 keys
    pool[5] = pool[9];
    std::vector<int> seen(pool.size(), 0), at(pool.size(), -1);
    for (int i = 0; i < (int)pool.size(); ++i) { const int r = rank(pool, i); ++seen[r]; at[r] = i; }
    for (size_t r = 0; r < pool.size(); ++r) expect(seen[r] == 1, "the ranks are a permutation", r, (uint64_t)seen[r]);
    for (size_t r = 0; r + 1 < pool.size(); ++r)
        if (at[r] >= 0 && at[r + 1] >= 0) {
            expect(!gymnet::key_less(pool[at[r]], pool[at[r + 1]]), "descending key by rank", r);
            if (same_key(pool[at[r]], pool[at[r + 1]])) expect(at[r] < at[r + 1], "equal keys by pool index", r);
        }
}

// merge_body after the selection: the keys that stay in the pool.  now: what is above the threshold key first, then what equals it
// (pool entries ahead of candidates) while there is room; before: every pool entry at or above the threshold, then the candidates at or
// above it in list order while there is room.
static std::vector<Key> merge_keys(const std::vector<Key> &pool, const std::vector<Key> &cand, uint32_t cap, bool now) {
    std::vector<Key> all = pool, out;
    all.insert(all.end(), cand.begin(), cand.end());
    if (all.size() <= cap) return all;
    const Key t = select_kth(all, cap);
    if (now) {
        for (const Key &k : all) if (gymnet::key_less(t, k)) out.push_back(k);
        for (const Key &k : all) if (same_key(t, k) && out.size() < cap) out.push_back(k);
    } else {
        for (const Key &k : pool) if (!gymnet::key_less(k, t)) out.push_back(k);
        for (const Key &k : cand) if (!gymnet::key_less(k, t) && out.size() < cap) out.push_back(k);
    }
    return out;
}

static void test_merge(bool now) {
    auto K = [](float r, uint64_t tick, int lane) { return key_of(Ep{r, tick, lane}); };
    struct Case { std::vector<Key> pool, cand; uint32_t cap; };
    const Case cases[] = {
        {{K(5, 1, 0), K(5, 1, 0)}, {K(7, 2, 1)}, 2},                                      // two equal at the threshold, a greater candidate
        {{K(5, 1, 0), K(5, 1, 0), K(9, 1, 3)}, {K(5, 1, 0), K(7, 2, 1), K(8, 2, 2)}, 3},
        {{K(5, 1, 0)}, {K(5, 1, 0), K(6, 1, 1)}, 2},                                      // the duplicate ahead of the greater key in the list
        {{K(1, 1, 0), K(2, 1, 0), K(3, 1, 0)}, {K(4, 2, 0), K(0, 2, 1)}, 3},              // no equal keys
        {{K(2, 3, 4), K(2, 3, 4), K(2, 3, 4)}, {K(2, 3, 4)}, 3},                          // all equal
    };
    for (const Case &c : cases) {
        std::vector<Key> all = c.pool, got = merge_keys(c.pool, c.cand, c.cap, now);
        all.insert(all.end(), c.cand.begin(), c.cand.end());
        auto desc = [](const Key &a, const Key &b) { return gymnet::key_before(a, b); };
        std::sort(all.begin(), all.end(), desc);
        std::sort(got.begin(), got.end(), desc);
        const size_t want = std::min<size_t>(all.size(), c.cap);
        bool ok = got.size() == want;
        for (size_t i = 0; ok && i < want; ++i) ok = same_key(got[i], all[i]);
        expect(ok, "the merge keeps the top-K multiset", c.cap, got.size());
    }
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--before") == 0) {
        struct { const char *name; void (*run)(); } rules[] = {
            {"predicate", [] { test_admission(admits_before); }},
            {"listing-order", [] { test_strict_weak_order(before_before, true); }},
            {"rank", [] { test_rank(rank_before); }},
            {"merge", [] { test_merge(false); }},
        };
        for (auto &r : rules) {
            g_checks = g_failed = 0;
            r.run();
            std::printf("before: %s %ld failed of %ld\n", r.name, g_failed, g_checks);
        }
        return 0;
    }
    test_ret_bits();
    test_key_less();
    test_selection();
    test_admission(gymnet::memory_admits);
    test_strict_weak_order(before_now, false);
    test_rank(rank_now);
    test_merge(true);
    std::printf("key: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
