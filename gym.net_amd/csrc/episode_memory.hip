// episode_memory.hip — the trainer's episode memory on the device: every step of every lane's open episode, the best `capacity`
// finished episodes by key (return, end tick, lane), and the dataset built from them (ReplayMemory.Memorize / EndEpisode,
// MemoryTypes/ReplayMemory.cs:25-67, and DataBuilder.BuildDataset, DataBuilders/DataBuilder.cs:25-55).  The contract is
// gymnet_vecenv_memory_config and its siblings in include/gymnet_amd.h; tests/_episode_memory_model.py restates it in NumPy.
// Written for gfx950 (wave64); compiled with -ffp-contract=off.
//
// Push (once per vector step, one thread per lane).  Steps are staged in a dense ring of L + 1 slots indexed by the memory's push
// count, so every lane writes the same slot and the stores coalesce like a recorded rollout's: slot s holds obs [D][N], action [N] and
// reward [N].  The step's action and reward go to slot pos, the post-step observation (the next step's o_p, or an auto-reset's o_0) to
// slot pos + 1; an episode of len <= L steps that ends at push pos occupies slots pos - len + 1 .. pos, and pos + 1 is never one of them.
// A lane whose episode ends compares its return with the pool's lowest kept return (read from the previous merge): a newer episode wins
// ties, so when the pool is full ret >= thr admits.  An episode whose return is NaN is never a candidate, whatever the pool holds
// (memory_admits, episode_memory_key.hpp): the pool, thr and the host's sort stay free of NaN.  Survivors are appended to the candidate
// list with one atomic per wave.
//
// Merge (a second launch, one workgroup; it returns at once when no episode was admitted, which is the common case after warm-up).  It
// keeps the top `capacity` keys of pool + candidates: a 16-digit radix select finds the K-th key, evicted pool blocks join the free
// list, and each winner copies its rows out of the ring into a free block [L][row].  Then it publishes the new threshold.  Keys can
// repeat (a tick set backwards, a replay after a restored checkpoint): the kept set is then the top-`capacity` MULTISET of keys — keys
// above the K-th stay or win first, keys equal to it fill what is left, pool entries ahead of candidates.
//
// Dataset (not per step): rank the kept keys (count of larger keys, and of equal keys at a lower pool index), scan the row counts floor(len * 2 / 3) in that order, then write
// params rows (one thread per row) or frames re-rendered from the stored observations with cartpole_raster.hpp (one wave per 1024
// pixels of one frame, as the pixel stack draws them).
//
// Rollout ingest (gymnet_vecenv_memory_push_rollout_device): the T recorded rows of one fused rollout go in as T pushes would, C steps
// per pass.  The ring then has L + C slots (ring_slots): an episode that ends at push pos still occupies pos - len + 1 .. pos, the pass
// writes at most slot pos + C, so nothing a merge of the pass needs is overwritten before it runs.  The scan kernel is the push kernel
// looped over the pass's steps with the lane's length and return in registers; step j's candidates go to segment j of the candidate list
// (its own counter), filtered against the pool as it stood before the pass — a threshold that is up to C steps stale only lets more
// candidates through.  The merge kernel then runs the merge once per segment in step order, so the kept set and `admitted` are those of
// T single pushes.
//
// The host side follows the kernels: gymnet_vecenv_memory_* and the handle's EpisodeMemory attachment.
#include <algorithm>
#include <type_traits>

#include "cartpole_raster.hpp"
#include "episode_memory_key.hpp"
#include "handle.hpp"

namespace gymnet {

namespace {

// A kept episode's key is (ret, tick, lane), ordered lexicographically; `block` is the pool block [L][row] that holds its steps.
struct MemEntry { float ret; int32_t len; uint64_t tick; int32_t lane, block; };
struct MemCand { float ret; int32_t len, lane, pad; };      // an episode that passed the push's admission filter
struct MemCtl {
    uint32_t cand_count;       // candidates of the most recent push (the merge consumes them and zeroes this); segment 0's of an ingest pass
    int32_t kept;              // pool entries [0, kept) are live
    int32_t full;              // kept == capacity: the push admits an ended episode only when ret >= thr
    float thr;                 // the lowest kept return (valid when full)
    uint64_t admitted;         // episodes the merges put into the pool
    uint64_t rows;             // dataset rows of the most recent dataset build
};                             // (the counters of candidate segments 1 .. C - 1 follow it in memory: seg_counter)
struct MemoryArgs {
    int64_t n;
    int32_t obs_dim, esz;                      // observation values per step and their size (4 float, 8 double)
    int32_t max_len, capacity;                 // L and K
    int32_t ring_slots, chunk;                 // L + C staging slots; C = steps per ingest pass (1: memory_config)
    // staging ring [L + C slots]: slot s at ring + s * slot_bytes holds obs [obs_dim][n] (esz each), action [n] (4 B), reward [n] (4 B)
    uint8_t *ring; int64_t slot_bytes;
    // pool: block b at pool + b * max_len * row_bytes, row p = obs [obs_dim] (esz each), action (4 B), reward (4 B)
    uint8_t *pool; int64_t row_bytes;
    int32_t *lane_len;                         // steps of the lane's open episode (-1: the lane is closed)
    float *lane_ret;                           // float32 sum of its rewards in step order
    MemCand *cand;                             // [C segments][n]
    MemCtl *ctl;
    MemEntry *meta, *meta_tmp;                 // [capacity] each: live entries, then free blocks
    int32_t *scratch;                          // [capacity]: free blocks during a merge, the descending key order during a dataset build
    int64_t *row_off;                          // [capacity + 1]: first dataset row of the episode of rank r
    uint64_t *partials;                        // [push_blocks][2]: episodes ended / too long, per push workgroup
    int32_t push_blocks;                       // workgroups of a push launch
};
struct MemPushArgs {
    const void *obs; int64_t obs_stride;       // the CURRENT observation buffer (after the step)
    const void *actions; const float *reward; const uint8_t *done;
    int64_t slot;                              // ring slot of this step (pos % ring_slots); the next step's is (pos + 1) % ring_slots
    uint64_t end_tick;                         // engine tick after the step: the key of the episodes that end in it
    int32_t autoreset;
};
// one ingest pass: steps t0 .. t0 + count - 1 of the buffers a rollout launch recorded
struct MemRolloutArgs {
    const void *rec_obs;                       // [steps][obs_dim][n]
    const uint32_t *actions; int64_t action_stride, ring;      // step t's actions: row (t % ring) * action_stride
    const float *rec_reward; const uint8_t *rec_done;          // [steps][n] each
    int64_t t0; int32_t count;                 // count <= chunk
    int64_t slot;                              // ring slot of step t0
    int32_t autoreset;
};
// format 0 = params rows, else GYMNET_STACK_* frames drawn as the pixel stack draws them (geo: their sample positions)
struct MemDatasetArgs {
    int32_t format, history;
    void *x; int32_t *action; float *onehot; float *reward;
    int64_t capacity_rows;
    int32_t action_n;                          // one-hot width (0: Box actions, no one-hot)
    FrameGeom geo;
};

__device__ __forceinline__ uint32_t wave_rank(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

constexpr int kPushBlock = 256;
constexpr int kMergeBlock = 1024;

// an empty pool: entry i owns block i, no counts, no candidates
__global__ __launch_bounds__(256) void memory_init_kernel(MemoryArgs m) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m.capacity) m.meta[i] = MemEntry{0.0f, 0, 0ull, -1, (int32_t)i};
    if (i < 2 * (int64_t)m.push_blocks) m.partials[i] = 0ull;
    if (i == 0) *m.ctl = MemCtl{};
    if (i < m.chunk - 1) reinterpret_cast<uint32_t *>(m.ctl + 1)[i] = 0u;
}

// the candidate counter of segment s of an ingest pass (segment 0's is the single push's)
__device__ __forceinline__ uint32_t *seg_counter(const MemoryArgs &m, int s) {
    return s == 0 ? &m.ctl->cand_count : reinterpret_cast<uint32_t *>(m.ctl + 1) + (s - 1);
}

template <class R>
__global__ __launch_bounds__(256) void memory_open_kernel(MemoryArgs m, const R *obs, int64_t ostride, const uint8_t *mask, int64_t slot) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m.n || (mask && !mask[k])) return;
    m.lane_len[k] = 0;
    m.lane_ret[k] = 0.0f;
    R *o = reinterpret_cast<R *>(m.ring + slot * m.slot_bytes);
    for (int d = 0; d < m.obs_dim; ++d) o[(int64_t)d * m.n + k] = obs[(int64_t)d * ostride + k];
}

template <class R>
__global__ __launch_bounds__(kPushBlock) void memory_push_kernel(MemoryArgs m, MemPushArgs p) {
    __shared__ uint32_t cnt[2];
    if (threadIdx.x == 0) { cnt[0] = 0u; cnt[1] = 0u; }
    __syncthreads();
    const int64_t k = (int64_t)blockIdx.x * kPushBlock + threadIdx.x;
    bool ended = false, too_long = false, cand = false;
    float ret = 0.0f;
    int32_t len = -1;
    if (k < m.n) len = m.lane_len[k];
    if (len >= 0) {
        const int64_t obs_bytes = (int64_t)m.obs_dim * m.n * (int64_t)sizeof(R);
        uint8_t *slot = m.ring + p.slot * m.slot_bytes;
        const uint32_t a = static_cast<const uint32_t *>(p.actions)[k];
        const float r = p.reward[k];
        const bool done = p.done[k] != 0;
        reinterpret_cast<uint32_t *>(slot + obs_bytes)[k] = a;
        reinterpret_cast<float *>(slot + obs_bytes + 4 * m.n)[k] = r;
        ret = m.lane_ret[k] + r;                          // the step kernel's EPISODE_STATS sum, in the same order
        len += 1;
        if (done) {
            ended = true;
            too_long = len > m.max_len;
            cand = memory_admits(too_long, m.ctl->full != 0, ret, m.ctl->thr);
        }
        if (!done || p.autoreset) {                       // the next step's o_p, or the auto-reset episode's o_0
            const int64_t nxt = p.slot + 1 == m.ring_slots ? 0 : p.slot + 1;
            R *o = reinterpret_cast<R *>(m.ring + nxt * m.slot_bytes);
            const R *src = static_cast<const R *>(p.obs);
            for (int d = 0; d < m.obs_dim; ++d) o[(int64_t)d * m.n + k] = src[(int64_t)d * p.obs_stride + k];
        }
        m.lane_len[k] = done ? (p.autoreset ? 0 : -1) : len;
        m.lane_ret[k] = done ? 0.0f : ret;
    }
    const int lid = threadIdx.x & 63;
    const uint64_t cm = __ballot(cand);
    if (cm) {
        const int leader = __ffsll((unsigned long long)cm) - 1;
        uint32_t base = 0;
        if (lid == leader) base = atomicAdd(&m.ctl->cand_count, (uint32_t)__popcll(cm));
        base = __shfl(base, leader);
        if (cand) m.cand[base + wave_rank(cm)] = MemCand{ret, len, (int32_t)k, 0};
    }
    const uint64_t em = __ballot(ended), tm = __ballot(too_long);
    if (lid == 0 && em) {
        atomicAdd(&cnt[0], (uint32_t)__popcll(em));
        if (tm) atomicAdd(&cnt[1], (uint32_t)__popcll(tm));
    }
    __syncthreads();
    if (threadIdx.x == 0 && cnt[0]) {                     // this workgroup's own counters: no contention
        m.partials[2 * blockIdx.x] += cnt[0];
        m.partials[2 * blockIdx.x + 1] += cnt[1];
    }
}

__device__ __forceinline__ Key entry_key(const MemoryArgs &m, const MemCand *cand, int64_t i, int32_t kept, uint64_t end_tick) {
    if (i < kept) { const MemEntry e = m.meta[i]; return make_key(e.ret, e.tick, e.lane); }
    const MemCand c = cand[i - kept];
    return make_key(c.ret, end_tick, c.lane);
}

// one merge by one workgroup of kMergeBlock: the candidates cand[0, *count) of the step staged in `slot`, whose episodes end at end_tick.
// REFILTER (the rollout ingest, whose scan filtered against the pool as it stood before the pass): a candidate counts only if it also
// passes the single push's filter against the pool as it stands now, so the merge sees exactly the candidates a single push would have
// made.  (A NaN return never gets this far: the scan's filter refuses it, as the push's does.)
template <int ESZ, bool REFILTER>
__device__ __forceinline__ void merge_body(const MemoryArgs &m, const MemCand *cand, uint32_t *count, int64_t slot, uint64_t end_tick) {
    using W = typename std::conditional<ESZ == 8, uint64_t, uint32_t>::type;
    __shared__ uint32_t hist[256];
    __shared__ uint32_t tau[4];
    __shared__ uint32_t need_s, min_bits;
    __shared__ int32_t n_keep, n_free, n_win, n_above, n_equal;
    const uint32_t cands = *count;
    if (cands == 0) return;
    const int32_t kept = m.ctl->kept, cap = m.capacity;
    const int32_t full_now = REFILTER ? m.ctl->full : 0;
    const float thr_now = REFILTER ? m.ctl->thr : 0.0f;
    auto counts = [&](const MemCand &c) { return !REFILTER || memory_admits(false, full_now != 0, c.ret, thr_now); };
    const int64_t total = (int64_t)kept + cands;
    // (REFILTER: total counts every candidate, so with a full pool the caller must have found one that counts — memory_merge_rollout_kernel's
    // pre-check — or the selection would look for a key that is not there)
    const bool select = total > cap;
    const int tid = threadIdx.x;
    if (tid < 4) tau[tid] = 0u;
    if (tid == 0) { need_s = (uint32_t)cap; min_bits = 0xFFFFFFFFu; n_keep = 0; n_free = 0; n_win = 0; n_above = 0; n_equal = 0; }
    __syncthreads();
    // the cap-th largest key: digit by digit, the bin where the count from the top reaches the rank still needed
    if (select) {
        for (int d = 0; d < 16; ++d) {
            if (tid < 256) hist[tid] = 0u;
            __syncthreads();
            const uint32_t t[4] = {tau[0], tau[1], tau[2], tau[3]};
            for (int64_t i = tid; i < total; i += kMergeBlock) {
                if (REFILTER && i >= kept && !counts(cand[i - kept])) continue;
                const Key k = entry_key(m, cand, i, kept, end_tick);
                if (prefix_match(k, t, d)) atomicAdd(&hist[digit(k, d)], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t cum = 0u;
                int b = 255;
                for (; b > 0; --b) {
                    if (cum + hist[b] >= need_s) break;
                    cum += hist[b];
                }
                need_s -= cum;
                tau[d >> 2] |= (uint32_t)b << (24 - 8 * (d & 3));
            }
            __syncthreads();
        }
    }
    Key t;
#pragma unroll
    for (int q = 0; q < 4; ++q) t.w[q] = tau[q];
    // After a selection t is the cap-th largest key.  Whatever is ABOVE it stays or wins; what EQUALS it (more than one entry only when keys
    // repeat: a tick set backwards, a replay from a restored checkpoint) takes the places that are left, pool entries ahead of candidates,
    // so a greater key is never dropped for an equal one and the kept set is the top-cap multiset of keys.
    if (select) {
        int32_t mine = 0;
        for (int64_t i = tid; i < total; i += kMergeBlock) {
            if (i >= kept && !counts(cand[i - kept])) continue;
            mine += key_less(t, entry_key(m, cand, i, kept, end_tick)) ? 1 : 0;
        }
        if (mine) atomicAdd(&n_above, mine);
        __syncthreads();
    }
    const int32_t room = cap - n_above;      // places for keys equal to t: at least one, t being the cap-th largest
    auto place = [&](const Key &k) {         // does this key stay in / enter the pool?
        if (!select) return true;
        if (key_less(k, t)) return false;
        return key_less(t, k) || atomicAdd(&n_equal, 1) < room;
    };
    // kept entries that have a place stay; the others' blocks, and the blocks of the unused entries, are free
    for (int i = tid; i < cap; i += kMergeBlock) {
        const MemEntry e = m.meta[i];
        if (i < kept && place(make_key(e.ret, e.tick, e.lane))) m.meta_tmp[atomicAdd(&n_keep, 1)] = e;
        else m.scratch[atomicAdd(&n_free, 1)] = e.block;
    }
    __syncthreads();
    const int32_t keep = n_keep;
    for (int64_t j = tid; j < cands; j += kMergeBlock) {
        const MemCand c = cand[j];
        if (counts(c) && place(make_key(c.ret, end_tick, c.lane))) {
            const int32_t s = atomicAdd(&n_win, 1);
            if (keep + s < cap) m.meta_tmp[keep + s] = MemEntry{c.ret, c.len, end_tick, c.lane, m.scratch[s]};
        }
    }
    __syncthreads();
    // exactly cap - keep candidates pass a selection (the places above t and the places equal to it add up to cap), and without one
    // kept + cands <= cap; the clamp only restates that bound where the blocks are handed out
    const int32_t win = n_win < cap - keep ? n_win : cap - keep, live = keep + win;
    for (int i = live + tid; i < cap; i += kMergeBlock) m.meta_tmp[i] = MemEntry{0.0f, 0, 0ull, -1, m.scratch[i - keep]};
    __syncthreads();
    for (int i = tid; i < cap; i += kMergeBlock) {
        const MemEntry e = m.meta_tmp[i];
        m.meta[i] = e;
        if (i < live) atomicMin(&min_bits, ret_bits(e.ret));
    }
    // each winner's rows out of the ring into its block: one wave per winner, a lane per row
    const int wave = tid >> 6, lid = tid & 63;
    const int64_t obs_bytes = (int64_t)m.obs_dim * m.n * ESZ;
    for (int w = wave; w < win; w += kMergeBlock / 64) {
        const MemEntry e = m.meta_tmp[keep + w];
        uint8_t *blk = m.pool + (int64_t)e.block * m.max_len * m.row_bytes;
        for (int q = lid; q < e.len; q += 64) {
            int64_t s = slot - e.len + 1 + q;
            if (s < 0) s += m.ring_slots;
            const uint8_t *src = m.ring + s * m.slot_bytes;
            uint8_t *row = blk + (int64_t)q * m.row_bytes;
            for (int d = 0; d < m.obs_dim; ++d)
                reinterpret_cast<W *>(row)[d] = reinterpret_cast<const W *>(src)[(int64_t)d * m.n + e.lane];
            reinterpret_cast<uint32_t *>(row + m.obs_dim * ESZ)[0] = reinterpret_cast<const uint32_t *>(src + obs_bytes)[e.lane];
            reinterpret_cast<uint32_t *>(row + m.obs_dim * ESZ)[1] = reinterpret_cast<const uint32_t *>(src + obs_bytes + 4 * m.n)[e.lane];
        }
    }
    __syncthreads();
    if (tid == 0) {
        m.ctl->kept = live;
        m.ctl->full = live == cap ? 1 : 0;
        m.ctl->thr = bits_ret(min_bits);
        m.ctl->admitted += (uint64_t)win;
        *count = 0u;
    }
}

template <int ESZ>
__global__ __launch_bounds__(kMergeBlock) void memory_merge_kernel(MemoryArgs m, int64_t slot, uint64_t end_tick) {
    merge_body<ESZ, false>(m, m.cand, &m.ctl->cand_count, slot, end_tick);
}

// The push kernel over the `count` steps of one ingest pass, reading the recorded rows instead of the handle's live arrays.  Step j's
// candidates go to segment j; the pool's full / thr are read once, as they stood before the pass.  The rows of step j + 1 are loaded
// into a second register set before step j's stores are issued.  (As compiled, the wait ahead of those stores covers the new loads too:
// they overlap the step's arithmetic, not its stores — docs/ledger.md §24.)
constexpr int kMemMaxObs = 8;      // observation values per step held in registers
static_assert(kMemMaxObs >= (int)(sizeof(EnvDesc::obs_low) / sizeof(float)), "the scan kernel holds every observation value an env can have");

template <class R>
__global__ __launch_bounds__(kPushBlock) void memory_scan_rollout_kernel(MemoryArgs m, MemRolloutArgs p) {
    __shared__ uint32_t cnt[2];
    if (threadIdx.x == 0) { cnt[0] = 0u; cnt[1] = 0u; }
    __syncthreads();
    const int64_t k = (int64_t)blockIdx.x * kPushBlock + threadIdx.x;
    const bool valid = k < m.n;
    const int lid = threadIdx.x & 63;
    const int D = m.obs_dim;
    const int64_t n = m.n, obs_bytes = (int64_t)D * n * (int64_t)sizeof(R);
    const R *rec_obs = static_cast<const R *>(p.rec_obs);
    const int32_t full = m.ctl->full;
    const float thr = m.ctl->thr;
    int32_t len = -1;
    float ret = 0.0f;
    if (valid) { len = m.lane_len[k]; ret = m.lane_ret[k]; }
    uint32_t ended_n = 0u, too_long_n = 0u;      // wave-uniform: episodes this wave ended in the pass
    // the rows of one step
    uint32_t a = 0u, a_nx = 0u;
    float r = 0.0f, r_nx = 0.0f;
    uint8_t dn = 0, dn_nx = 0;
    R o[kMemMaxObs], o_nx[kMemMaxObs];
#pragma unroll
    for (int d = 0; d < kMemMaxObs; ++d) { o[d] = R(0); o_nx[d] = R(0); }
    int64_t ring_i = p.t0 % p.ring;              // the action row of the next step to load
    auto load = [&](int64_t t, uint32_t &aa, float &rr, uint8_t &dd, R (&oo)[kMemMaxObs]) {
        const int64_t arow = ring_i * p.action_stride;
        ring_i = ring_i + 1 == p.ring ? 0 : ring_i + 1;
        if (!valid) return;
        aa = p.actions[arow + k];
        rr = p.rec_reward[t * n + k];
        dd = p.rec_done[t * n + k];
        const R *row = rec_obs + t * D * n + k;
#pragma unroll
        for (int d = 0; d < kMemMaxObs; ++d)
            if (d < D) oo[d] = row[(int64_t)d * n];
    };
    load(p.t0, a, r, dn, o);
    int64_t slot = p.slot;
    for (int j = 0; j < p.count; ++j) {
        if (j + 1 < p.count) load(p.t0 + j + 1, a_nx, r_nx, dn_nx, o_nx);
        const int64_t nxt = slot + 1 == m.ring_slots ? 0 : slot + 1;
        bool ended = false, too_long = false, cand = false;
        float ep_ret = 0.0f;
        int32_t ep_len = 0;
        if (len >= 0) {
            uint8_t *sp = m.ring + slot * m.slot_bytes;
            const bool done = dn != 0;
            reinterpret_cast<uint32_t *>(sp + obs_bytes)[k] = a;
            reinterpret_cast<float *>(sp + obs_bytes + 4 * n)[k] = r;
            ret += r;
            len += 1;
            if (done) {
                ended = true;
                too_long = len > m.max_len;
                cand = memory_admits(too_long, full != 0, ret, thr);
                ep_ret = ret; ep_len = len;
            }
            if (!done || p.autoreset) {
                R *on = reinterpret_cast<R *>(m.ring + nxt * m.slot_bytes);
#pragma unroll
                for (int d = 0; d < kMemMaxObs; ++d)
                    if (d < D) on[(int64_t)d * n + k] = o[d];
            }
            if (done) { len = p.autoreset ? 0 : -1; ret = 0.0f; }
        }
        const uint64_t cm = __ballot(cand);
        if (cm) {
            const int leader = __ffsll((unsigned long long)cm) - 1;
            uint32_t base = 0;
            if (lid == leader) base = atomicAdd(seg_counter(m, j), (uint32_t)__popcll(cm));
            base = __shfl(base, leader);
            if (cand) m.cand[(int64_t)j * n + base + wave_rank(cm)] = MemCand{ep_ret, ep_len, (int32_t)k, 0};
        }
        ended_n += (uint32_t)__popcll(__ballot(ended));
        too_long_n += (uint32_t)__popcll(__ballot(too_long));
        slot = nxt;
        a = a_nx; r = r_nx; dn = dn_nx;
#pragma unroll
        for (int d = 0; d < kMemMaxObs; ++d) o[d] = o_nx[d];
    }
    if (valid) { m.lane_len[k] = len; m.lane_ret[k] = ret; }
    if (lid == 0 && ended_n) {
        atomicAdd(&cnt[0], ended_n);
        if (too_long_n) atomicAdd(&cnt[1], too_long_n);
    }
    __syncthreads();
    if (threadIdx.x == 0 && cnt[0]) {
        m.partials[2 * blockIdx.x] += cnt[0];
        m.partials[2 * blockIdx.x + 1] += cnt[1];
    }
}

// `count` merges in step order: segment j holds the candidates of the step staged in slot + j, whose episodes end at end_tick + j * dtick.
// The scan filtered them against the pool as it stood before the pass; a segment none of whose candidates passes the single push's
// filter against the pool as it stands NOW (full, and every return below the lowest kept) cannot change the pool and is dropped
// without a selection.
template <int ESZ>
__global__ __launch_bounds__(kMergeBlock) void memory_merge_rollout_kernel(MemoryArgs m, int64_t slot, uint64_t end_tick, uint64_t dtick,
                                                                            int32_t count) {
    __shared__ uint32_t pass;
    for (int j = 0; j < count; ++j) {
        uint32_t *counter = seg_counter(m, j);
        const uint32_t cands = *counter;         // (uniform: only this segment's turn zeroes it, behind a barrier)
        if (cands != 0u) {
            const MemCand *cand = m.cand + (int64_t)j * m.n;
            if (threadIdx.x == 0) pass = 0u;
            __syncthreads();
            const int32_t full = m.ctl->full;
            const float thr = m.ctl->thr;
            bool any = false;
            for (uint32_t i = threadIdx.x; i < cands; i += kMergeBlock) any |= memory_admits(false, full != 0, cand[i].ret, thr);
            if (any) pass = 1u;
            __syncthreads();
            if (pass) {
                int64_t s = slot + j;
                if (s >= m.ring_slots) s -= m.ring_slots;
                merge_body<ESZ, true>(m, cand, counter, s, end_tick + (uint64_t)j * dtick);
            } else if (threadIdx.x == 0) {
                *counter = 0u;
            }
        }
        __syncthreads();                         // the next merge reads the pool and the control block this one wrote
    }
}

// ---- dataset -----------------------------------------------------------------------------------------------------------------

// scratch[rank] = the entry of that rank, 0 the largest key; equal keys rank by pool index, so scratch[0, kept) is a permutation
__global__ __launch_bounds__(256) void memory_rank_kernel(MemoryArgs m) {
    const int32_t kept = m.ctl->kept;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kept) return;
    const MemEntry e = m.meta[i];
    const Key ki = make_key(e.ret, e.tick, e.lane);
    int r = 0;
    for (int j = 0; j < kept; ++j) {
        const MemEntry f = m.meta[j];
        r += key_ranks_before(make_key(f.ret, f.tick, f.lane), j, ki, i) ? 1 : 0;
    }
    m.scratch[r] = i;
}

__device__ __forceinline__ int64_t rows_of(int32_t len) { return (int64_t)len * 2 / 3; }     // DataBuilder.cs:33

// row_off[r] = first row of the episode of rank r, row_off[kept] = ctl->rows = every row
__global__ __launch_bounds__(1024) void memory_scan_kernel(MemoryArgs m) {
    __shared__ int64_t part[1024];
    const int32_t kept = m.ctl->kept;
    const int tid = threadIdx.x;
    const int per = (kept + 1023) / 1024;
    const int lo = tid * per, hi = lo + per < kept ? lo + per : kept;
    int64_t s = 0;
    for (int r = lo; r < hi; ++r) s += rows_of(m.meta[m.scratch[r]].len);
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int64_t acc = 0;
        for (int q = 0; q < 1024; ++q) { const int64_t v = part[q]; part[q] = acc; acc += v; }
        m.row_off[kept] = acc;
        m.ctl->rows = (uint64_t)acc;
    }
    __syncthreads();
    int64_t off = part[tid];
    for (int r = lo; r < hi; ++r) { m.row_off[r] = off; off += rows_of(m.meta[m.scratch[r]].len); }
}

// the episode (rank) a dataset row belongs to: the largest r with row_off[r] <= row
__device__ __forceinline__ int find_rank(const int64_t *row_off, int32_t kept, int64_t row) {
    int lo = 0, hi = kept - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (row_off[mid] <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <class R>
__global__ __launch_bounds__(256) void memory_rows_kernel(MemoryArgs m, MemDatasetArgs d) {
    const int32_t kept = m.ctl->kept;
    const int64_t total = m.row_off[kept];
    const int64_t lim = total < d.capacity_rows ? total : d.capacity_rows;
    const int S = d.history, D = m.obs_dim;
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < lim; row += (int64_t)gridDim.x * 256) {
        const int r = find_rank(m.row_off, kept, row);
        const MemEntry e = m.meta[m.scratch[r]];
        const int64_t p = row - m.row_off[r];
        const uint8_t *blk = m.pool + (int64_t)e.block * m.max_len * m.row_bytes;
        const uint8_t *rp = blk + p * m.row_bytes;
        const uint32_t a = reinterpret_cast<const uint32_t *>(rp + D * sizeof(R))[0];
        if (d.action) d.action[row] = (int32_t)a;
        if (d.reward) d.reward[row] = reinterpret_cast<const float *>(rp + D * sizeof(R))[1];
        if (d.onehot)
            for (int j = 0; j < d.action_n; ++j) d.onehot[row * d.action_n + j] = (uint32_t)j == a ? 1.0f : 0.0f;
        if (d.format == 0 && d.x) {
            float *x = static_cast<float *>(d.x) + row * (int64_t)S * D;
            for (int s = 0; s < S; ++s) {
                const int64_t q = p - (S - 1) + s;
                const R *o = reinterpret_cast<const R *>(blk + (q > 0 ? q : 0) * m.row_bytes);
                for (int c = 0; c < D; ++c) x[s * D + c] = (float)o[c];
            }
        }
    }
}

template <class R, int FMT>
__global__ __launch_bounds__(256) void memory_frames_kernel(MemoryArgs m, MemDatasetArgs d) {
    constexpr int E = FMT == GYMNET_STACK_BINARY_F32 ? 4 : 1;
    const int32_t kept = m.ctl->kept;
    const int64_t total = m.row_off[kept];
    const int64_t lim = total < d.capacity_rows ? total : d.capacity_rows;
    const int S = d.history;
    const int64_t frame_px = (int64_t)d.geo.out_w * d.geo.out_h;
    const int64_t total_waves = lim * S * d.geo.waves_per_frame;
    const int lid = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t w = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); w < total_waves; w += nwaves) {
        const int64_t f = w / d.geo.waves_per_frame, slice = w - f * d.geo.waves_per_frame;
        const int64_t row = f / S;
        const int s = (int)(f - row * S);
        const int64_t p0 = slice * kPixPerWave + (int64_t)lid * kPixPerThread;
        if (p0 >= frame_px) continue;
        const int r = find_rank(m.row_off, kept, row);
        const MemEntry e = m.meta[m.scratch[r]];
        const int64_t q = row - m.row_off[r] - (S - 1) + s;
        const R *o = reinterpret_cast<const R *>(m.pool + ((int64_t)e.block * m.max_len + (q > 0 ? q : 0)) * m.row_bytes);
        const Geo g = lane_geometry(o, 1, 0);
        int i = (int)(p0 / d.geo.out_w), j = (int)(p0 - (int64_t)i * d.geo.out_w);
        uint8_t *out = static_cast<uint8_t *>(d.x) + (f * frame_px + p0) * E;
        const int cnt = frame_px - p0 < kPixPerThread ? (int)(frame_px - p0) : kPixPerThread;
#pragma unroll 1
        for (int v = 0; v < cnt; ++v) {
            int nw, np;
            shade(g, d.geo.x0, d.geo.sxq, d.geo.y0, d.geo.syq, i, j, nw, np);
            const uint32_t val = stack_value<FMT>(nw, np);
            if constexpr (E == 4) reinterpret_cast<uint32_t *>(out)[v] = val;
            else out[v] = (uint8_t)val;
            if (++j == d.geo.out_w) { j = 0; ++i; }
        }
    }
}

unsigned grid_for(int64_t items, int64_t per_block, int64_t max_blocks) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b < max_blocks ? b : max_blocks));
}

template <class R>
hipError_t launch_dataset_typed(const MemoryArgs &m, const MemDatasetArgs &d, hipStream_t st) {
    hipLaunchKernelGGL(memory_rank_kernel, dim3(grid_for(m.capacity, 256, 1 << 20)), dim3(256), 0, st, m);
    hipLaunchKernelGGL(memory_scan_kernel, dim3(1), dim3(1024), 0, st, m);
    hipLaunchKernelGGL((memory_rows_kernel<R>), dim3(grid_for(d.capacity_rows, 256, 1 << 14)), dim3(256), 0, st, m, d);
    if (d.format != 0 && d.x) {
        const unsigned g = grid_for(d.capacity_rows * d.history * d.geo.waves_per_frame, 4, 1 << 16);
        if (d.format == GYMNET_STACK_GRAY8) hipLaunchKernelGGL((memory_frames_kernel<R, GYMNET_STACK_GRAY8>), dim3(g), dim3(256), 0, st, m, d);
        else if (d.format == GYMNET_STACK_BINARY8) hipLaunchKernelGGL((memory_frames_kernel<R, GYMNET_STACK_BINARY8>), dim3(g), dim3(256), 0, st, m, d);
        else hipLaunchKernelGGL((memory_frames_kernel<R, GYMNET_STACK_BINARY_F32>), dim3(g), dim3(256), 0, st, m, d);
    }
    return hipGetLastError();
}

// an empty pool, zero counts
hipError_t launch_memory_init(const MemoryArgs &m, hipStream_t st) {
    const int64_t items = m.capacity > 2 * (int64_t)m.push_blocks ? m.capacity : 2 * (int64_t)m.push_blocks;
    hipLaunchKernelGGL(memory_init_kernel, dim3(grid_for(items, 256, INT32_MAX)), dim3(256), 0, st, m);
    return hipGetLastError();
}

hipError_t launch_memory_open(bool f64, const MemoryArgs &m, const void *obs, int64_t obs_stride, const uint8_t *mask, int64_t slot,
                              hipStream_t st) {
    const unsigned g = grid_for(m.n, 256, INT32_MAX);
    if (f64) hipLaunchKernelGGL(memory_open_kernel<double>, dim3(g), dim3(256), 0, st, m, static_cast<const double *>(obs), obs_stride, mask, slot);
    else hipLaunchKernelGGL(memory_open_kernel<float>, dim3(g), dim3(256), 0, st, m, static_cast<const float *>(obs), obs_stride, mask, slot);
    return hipGetLastError();
}

hipError_t launch_memory_push(bool f64, const MemoryArgs &m, const MemPushArgs &p, hipStream_t st) {
    if (f64) {
        hipLaunchKernelGGL(memory_push_kernel<double>, dim3(m.push_blocks), dim3(kPushBlock), 0, st, m, p);
        hipLaunchKernelGGL(memory_merge_kernel<8>, dim3(1), dim3(kMergeBlock), 0, st, m, p.slot, p.end_tick);
    } else {
        hipLaunchKernelGGL(memory_push_kernel<float>, dim3(m.push_blocks), dim3(kPushBlock), 0, st, m, p);
        hipLaunchKernelGGL(memory_merge_kernel<4>, dim3(1), dim3(kMergeBlock), 0, st, m, p.slot, p.end_tick);
    }
    return hipGetLastError();
}

// one ingest pass: the scan over p.count steps, then their merges; dtick = engine ticks per step
hipError_t launch_memory_push_rollout(bool f64, const MemoryArgs &m, const MemRolloutArgs &p, uint64_t end_tick, uint64_t dtick, hipStream_t st) {
    if (f64) {
        hipLaunchKernelGGL(memory_scan_rollout_kernel<double>, dim3(m.push_blocks), dim3(kPushBlock), 0, st, m, p);
        hipLaunchKernelGGL(memory_merge_rollout_kernel<8>, dim3(1), dim3(kMergeBlock), 0, st, m, p.slot, end_tick, dtick, p.count);
    } else {
        hipLaunchKernelGGL(memory_scan_rollout_kernel<float>, dim3(m.push_blocks), dim3(kPushBlock), 0, st, m, p);
        hipLaunchKernelGGL(memory_merge_rollout_kernel<4>, dim3(1), dim3(kMergeBlock), 0, st, m, p.slot, end_tick, dtick, p.count);
    }
    return hipGetLastError();
}

constexpr int32_t kMemoryMaxCapacity = 65536;
constexpr int32_t kMemoryMaxHistory = 64;
constexpr int32_t kMemoryMaxLength = 1 << 24;
constexpr int32_t kMemoryMaxChunk = 64;

}  // namespace

// the configured memory: pos counts its pushes (the ring slot of the next step is pos % ring_slots); last: the handle's step counters
// at its last config, reset or push, so a push can tell that exactly one vector step ran in between; last_tick: the engine tick then
// (an ingest reads the launch's ticks per decision off it)
struct EpisodeMemory {
    DeviceAllocs mem; MemoryArgs args{}; int32_t history = 0; uint64_t pos = 0; StepMark last; uint64_t last_tick = 0;
    void mark_now(const gymnet_vecenv *h) { last = mark(h); last_tick = h->tick; }
};

int release_memory(gymnet_vecenv *h) { return release_attachment(h, h->memory); }

namespace {

int need_memory(gymnet_vecenv *h) {
    return h->memory ? GYMNET_OK : fail(h, GYMNET_ERR_INVALID_ARG, "no episode memory configured (gymnet_vecenv_memory_config)");
}

int64_t ring_slot(const EpisodeMemory &em) { return (int64_t)(em.pos % (uint64_t)em.args.ring_slots); }

// the kept entries [0, kept) and the control block, read back after the stream has drained
int read_pool(gymnet_vecenv *h, MemCtl *ctl, std::vector<MemEntry> *meta) {
    const MemoryArgs &m = h->memory->args;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(ctl, m.ctl, sizeof *ctl, hipMemcpyDeviceToHost));
    if (meta) {
        meta->resize((size_t)ctl->kept);
        if (ctl->kept > 0) HIP_TRY(h, hipMemcpy(meta->data(), m.meta, sizeof(MemEntry) * (size_t)ctl->kept, hipMemcpyDeviceToHost));
    }
    return GYMNET_OK;
}

// a push of `asked` steps is accepted after exactly one step launch of that many decisions
int check_push_follows(gymnet_vecenv *h, const EpisodeMemory &em, int64_t asked) {
    const StepMark s = since(h, em.last);
    if (asked >= 1 && s == StepMark{(uint64_t)asked, 1}) return GYMNET_OK;
    return fail(h, GYMNET_ERR_INVALID_ARG, "a push needs exactly one vector step since the last memory config, reset or push (tick %llu -> %llu, "
                "%llu step launches); after a reset of the handle call gymnet_vecenv_memory_reset_device [%llu step(s) seen, %lld asked: a "
                "launch of several steps goes in through gymnet_vecenv_memory_push_rollout_device; %llu reset / seed / set_tick / set_state calls "
                "of the handle since: any makes the memory stale]", (unsigned long long)em.last.tick,
                (unsigned long long)(h->tick - h->held_ticks), (unsigned long long)s.launches, (unsigned long long)s.tick,
                (long long)asked, (unsigned long long)s.epoch);   // (ticks on the decision clock: StepMark)
}

// gymnet_vecenv_memory_config (chunk 1) and gymnet_vecenv_memory_config_rollout, on a handle the caller has ENTERed
int memory_configure(gymnet_vecenv *h, int32_t capacity, int32_t max_length, int32_t history, int32_t chunk) {
    if (capacity == 0) return release_memory(h);
    if (capacity < 0 || capacity > kMemoryMaxCapacity)
        return fail(h, GYMNET_ERR_INVALID_ARG, "capacity %d not in [0, %d]", capacity, kMemoryMaxCapacity);
    if (history < 1 || history > kMemoryMaxHistory) return fail(h, GYMNET_ERR_INVALID_ARG, "history %d not in [1, %d]", history, kMemoryMaxHistory);
    const int32_t len = max_length == 0 ? h->cfg.max_episode_steps : max_length;
    if (max_length < 0 || len < 1 || len > kMemoryMaxLength)
        return fail(h, GYMNET_ERR_INVALID_ARG, "max_length %d not in [1, %d] (0 = max_episode_steps, which is %d)", max_length, kMemoryMaxLength,
                    h->cfg.max_episode_steps);
    const int obs_dim = h->desc->obs_dim;
    const int64_t row = (int64_t)obs_dim * (int64_t)h->esz + 8;
    const double ring_d = (double)(len + chunk) * (double)h->n * (double)row, pool_d = (double)capacity * (double)len * (double)row;
    if (ring_d > 9.0e18 || pool_d > 9.0e18) return fail(h, GYMNET_ERR_INVALID_ARG, "episode memory of %.3g bytes overflows", ring_d + pool_d);
    std::unique_ptr<EpisodeMemory> fresh(new EpisodeMemory);
    MemoryArgs &m = fresh->args;
    m.n = h->n; m.obs_dim = obs_dim; m.esz = (int32_t)h->esz;
    m.max_len = len; m.capacity = capacity;
    m.ring_slots = len + chunk; m.chunk = chunk;
    m.slot_bytes = h->n * row; m.row_bytes = row;
    m.push_blocks = (int32_t)((h->n + kPushBlock - 1) / kPushBlock);
    // every region (ring, pool, per-lane state, candidates, control, pool entries, scratch, row offsets, counters) or none
    bool ok = true;
    auto take = [&](auto *&p, int64_t bytes) {
        using P = std::remove_reference_t<decltype(p)>;
        ok = ok && (p = static_cast<P>(fresh->mem.take((size_t)bytes))) != nullptr;
    };
    take(m.ring, (int64_t)m.ring_slots * m.slot_bytes); take(m.pool, (int64_t)capacity * len * row);
    take(m.lane_len, 4 * h->n); take(m.lane_ret, 4 * h->n); take(m.cand, (int64_t)sizeof(MemCand) * h->n * chunk);
    take(m.ctl, sizeof(MemCtl) + 4 * (int64_t)(chunk - 1)); take(m.meta, (int64_t)sizeof(MemEntry) * capacity);
    take(m.meta_tmp, (int64_t)sizeof(MemEntry) * capacity); take(m.scratch, 4 * (int64_t)capacity);
    take(m.row_off, 8 * ((int64_t)capacity + 1)); take(m.partials, 16 * (int64_t)m.push_blocks);
    if (!ok) return fail(h, GYMNET_ERR_OOM, "hipMalloc of the episode memory (%.3g bytes) failed", ring_d + pool_d);
    fresh->history = history;
    fresh->mark_now(h);
    ST_TRY(release_memory(h));
    h->memory = fresh.release();
    HIP_TRY(h, launch_memory_init(m, h->stream));
    HIP_TRY(h, launch_memory_open(h->f64, m, h->d_obs, h->ostride, nullptr, 0, h->stream));
    return GYMNET_OK;
}

}  // namespace

}  // namespace gymnet

using namespace gymnet;

extern "C" {

int gymnet_vecenv_memory_config(gymnet_vecenv *h, int32_t capacity, int32_t max_length, int32_t history) {
    return guarded([&]() -> int {
    ENTER(h);
    return memory_configure(h, capacity, max_length, history, 1);
    });
}

int gymnet_vecenv_memory_config_rollout(gymnet_vecenv *h, int32_t capacity, int32_t max_length, int32_t history, int32_t rollout_chunk) {
    return guarded([&]() -> int {
    ENTER(h);
    if (rollout_chunk < 1 || rollout_chunk > kMemoryMaxChunk)
        return fail(h, GYMNET_ERR_INVALID_ARG, "rollout_chunk %d not in [1, %d]", rollout_chunk, kMemoryMaxChunk);
    return memory_configure(h, capacity, max_length, history, rollout_chunk);
    });
}

int gymnet_vecenv_memory_reset_device(gymnet_vecenv *h, const uint8_t *d_mask, int32_t clear_pool) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_memory(h));
    EpisodeMemory &em = *h->memory;
    if (clear_pool) HIP_TRY(h, launch_memory_init(em.args, h->stream));
    HIP_TRY(h, launch_memory_open(h->f64, em.args, h->d_obs, h->ostride, d_mask, ring_slot(em), h->stream));
    em.mark_now(h);
    return GYMNET_OK;
    });
}

int gymnet_vecenv_memory_push_device(gymnet_vecenv *h, const void *d_actions, const uint8_t *d_done) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_memory(h));
    EpisodeMemory &em = *h->memory;
    if (!d_actions) return fail(h, GYMNET_ERR_INVALID_ARG, "d_actions is null");
    ST_TRY(check_push_follows(h, em, 1));
    MemPushArgs p{};
    p.obs = h->d_obs; p.obs_stride = h->ostride;
    p.actions = d_actions; p.reward = h->d_reward; p.done = d_done ? d_done : h->d_done;
    p.slot = ring_slot(em);
    p.end_tick = h->tick;
    p.autoreset = h->autoreset ? 1 : 0;
    HIP_TRY(h, launch_memory_push(h->f64, em.args, p, h->stream));
    em.pos += 1;
    em.mark_now(h);
    return GYMNET_OK;
    });
}

int gymnet_vecenv_memory_push_rollout_device(gymnet_vecenv *h, int64_t steps, const void *d_rec_obs, const void *d_actions,
                                             int64_t action_stride, int64_t ring, const float *d_rec_reward, const uint8_t *d_rec_done) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_memory(h));
    EpisodeMemory &em = *h->memory;
    if (!d_rec_obs || !d_actions || !d_rec_reward || !d_rec_done)
        return fail(h, GYMNET_ERR_INVALID_ARG, "d_rec_obs, d_actions, d_rec_reward or d_rec_done is null");
    if (steps < 1 || ring < 1 || action_stride < 0)
        return fail(h, GYMNET_ERR_INVALID_ARG, "bad steps/ring/action_stride (%lld, %lld, %lld)", (long long)steps, (long long)ring, (long long)action_stride);
    // the launch's engine ticks per decision (frame skip: R sub-steps each): row t ends at tick_before + (t + 1) * R.  One launch moves
    // the engine tick by steps * R, so any other distance over the right number of decisions means set_tick came in between; that is
    // said in its own words, ahead of the staleness gate (which refuses every set_tick, this one included)
    const uint64_t ticks = h->tick - em.last_tick;
    const StepMark moved = since(h, em.last);
    if (moved.tick == (uint64_t)steps && moved.launches == 1 && (ticks < (uint64_t)steps || ticks % (uint64_t)steps != 0))
        return fail(h, GYMNET_ERR_INVALID_ARG, "the tick moved by %llu over %lld steps: not one launch's", (unsigned long long)ticks, (long long)steps);
    ST_TRY(check_push_follows(h, em, steps));
    const uint64_t dtick = ticks / (uint64_t)steps;
    MemRolloutArgs p{};
    p.rec_obs = d_rec_obs; p.actions = static_cast<const uint32_t *>(d_actions); p.action_stride = action_stride; p.ring = ring;
    p.rec_reward = d_rec_reward; p.rec_done = d_rec_done;
    p.autoreset = h->autoreset ? 1 : 0;
    for (int64_t t0 = 0; t0 < steps; t0 += em.args.chunk) {
        p.t0 = t0;
        p.count = (int32_t)std::min<int64_t>(em.args.chunk, steps - t0);
        p.slot = ring_slot(em);
        HIP_TRY(h, launch_memory_push_rollout(h->f64, em.args, p, em.last_tick + (uint64_t)(t0 + 1) * dtick, dtick, h->stream));
        em.pos += (uint64_t)p.count;
    }
    em.mark_now(h);
    return GYMNET_OK;
    });
}

int gymnet_vecenv_memory_stats(gymnet_vecenv *h, int64_t *kept, int64_t *ended, int64_t *admitted, int64_t *too_long) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_memory(h));
    MemCtl ctl{};
    ST_TRY(read_pool(h, &ctl, nullptr));
    std::vector<uint64_t> part((size_t)h->memory->args.push_blocks * 2);
    HIP_TRY(h, hipMemcpy(part.data(), h->memory->args.partials, part.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    uint64_t e = 0, t = 0;
    for (size_t b = 0; b < part.size(); b += 2) { e += part[b]; t += part[b + 1]; }
    if (kept) *kept = ctl.kept;
    if (ended) *ended = (int64_t)e;
    if (admitted) *admitted = (int64_t)ctl.admitted;
    if (too_long) *too_long = (int64_t)t;
    return GYMNET_OK;
    });
}

int gymnet_vecenv_memory_episodes(gymnet_vecenv *h, float *ret, int32_t *len, uint64_t *end_tick, int32_t *lane, int64_t capacity,
                                  int64_t *count) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_memory(h));
    if (capacity < 0) return fail(h, GYMNET_ERR_INVALID_ARG, "capacity %lld < 0", (long long)capacity);
    MemCtl ctl{};
    std::vector<MemEntry> meta;
    ST_TRY(read_pool(h, &ctl, &meta));
    // descending key (return, tick, lane); equal keys in pool order, as the dataset ranks them
    std::stable_sort(meta.begin(), meta.end(), [](const MemEntry &a, const MemEntry &b) {
        return key_before(make_key(a.ret, a.tick, a.lane), make_key(b.ret, b.tick, b.lane));
    });
    const int64_t m = (int64_t)meta.size() < capacity ? (int64_t)meta.size() : capacity;
    for (int64_t i = 0; i < m; ++i) {
        if (ret) ret[i] = meta[(size_t)i].ret;
        if (len) len[i] = meta[(size_t)i].len;
        if (end_tick) end_tick[i] = meta[(size_t)i].tick;
        if (lane) lane[i] = meta[(size_t)i].lane;
    }
    if (count) *count = (int64_t)meta.size();
    return GYMNET_OK;
    });
}

int gymnet_vecenv_memory_dataset_size(gymnet_vecenv *h, int64_t *rows) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_memory(h));
    if (!rows) return fail(h, GYMNET_ERR_INVALID_ARG, "rows is null");
    MemCtl ctl{};
    std::vector<MemEntry> meta;
    ST_TRY(read_pool(h, &ctl, &meta));
    int64_t r = 0;
    for (const MemEntry &e : meta) r += (int64_t)e.len * 2 / 3;
    *rows = r;
    return GYMNET_OK;
    });
}

int gymnet_vecenv_memory_dataset_device(gymnet_vecenv *h, int32_t format, int32_t crop_x, int32_t crop_y, int32_t crop_w, int32_t crop_h,
                                        int32_t out_w, int32_t out_h, void *d_x, int32_t *d_action, float *d_onehot, float *d_reward,
                                        int64_t capacity_rows) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_memory(h));
    if (format != GYMNET_MEMORY_PARAMS && format != GYMNET_STACK_GRAY8 && format != GYMNET_STACK_BINARY8 && format != GYMNET_STACK_BINARY_F32)
        return fail(h, GYMNET_ERR_INVALID_ARG, "unknown dataset format %d", format);
    if (format != GYMNET_MEMORY_PARAMS) {
        if (h->cfg.env_id != GYMNET_ENV_CARTPOLE) return fail(h, GYMNET_ERR_UNSUPPORTED, "pixel datasets exist for CartPole only (CartPoleEnv.cs:69-135)");
        ST_TRY(check_crop_and_size(h, crop_x, crop_y, crop_w, crop_h, out_w, out_h));
    }
    if (capacity_rows < 0) return fail(h, GYMNET_ERR_INVALID_ARG, "capacity_rows %lld < 0", (long long)capacity_rows);
    if (d_onehot && h->desc->box_action) return fail(h, GYMNET_ERR_INVALID_ARG, "a Box action has no one-hot");
    if (format == GYMNET_STACK_BINARY_F32 && !aligned_to(d_x, 4)) return fail(h, GYMNET_ERR_INVALID_ARG, "BINARY_F32 rows need a 4-byte aligned d_x");
    if (capacity_rows == 0) return GYMNET_OK;
    MemDatasetArgs d{};
    d.format = format; d.history = h->memory->history;
    d.x = d_x; d.action = d_action; d.onehot = d_onehot; d.reward = d_reward;
    d.capacity_rows = capacity_rows;
    d.action_n = h->desc->box_action ? 0 : h->desc->action_n;
    if (format != GYMNET_MEMORY_PARAMS) d.geo = frame_geom(crop_x, crop_y, crop_w, crop_h, out_w, out_h);
    const MemoryArgs &m = h->memory->args;
    HIP_TRY(h, h->f64 ? launch_dataset_typed<double>(m, d, h->stream) : launch_dataset_typed<float>(m, d, h->stream));
    return GYMNET_OK;
    });
}

}  // extern "C"
