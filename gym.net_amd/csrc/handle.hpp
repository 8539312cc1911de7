// handle.hpp — what a gymnet_vecenv handle IS, plus the host-side helpers the library's units share.  capi.hip holds the C entry points
// of the handle itself and the host boundary; three subsystems with state of their own on the handle have a unit each —
// launch_policy.hip (h->lcfg and what may replace it), resident.hip (h->res: the mailbox and its kernel), step_graph.hip (h->graph: the
// captured rollouts) — beside group.hip and the attachment units.  The fused rollout has rollout_fused.hip (h->ep: the episode-segment
// block; what a call will do is rollout_plan.hpp's pure function), frame skip's entry points sit beside its kernels in action_repeat.hip.
// Internal to the library: nothing here crosses the C ABI (include/gymnet_amd.h is the boundary).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/gymnet_amd.h"
#include "kernels.hpp"

namespace gymnet {

struct EnvDesc {
    const char *name;
    int state_dim, obs_dim;
    bool alias, box_action, has_sbd;
    int action_n;
    float action_low, action_high;
    float obs_low[8], obs_high[8];
    float reward_low, reward_high;
    int algorithmic_bytes;
    int traffic_bytes;          // bytes one env-step really moves (< algorithmic where a state row is stored once, in the observation)
    int state_row_in_obs[4];    // state row k lives in observation row state_row_in_obs[k] (-1: its own row of the state array)
};
extern const EnvDesc kEnvs[kNumEnvs];

// GYMNET_FLAG_RESIDENT (num_envs <= 64): the mailbox in coherent host memory and the state of the resident kernel (resident.hip)
struct Resident {
    Mailbox *mb = nullptr;         // host address (page-locked, device-mapped, coherent)
    Mailbox *mb_dev = nullptr;     // the same memory as the device sees it
    bool enabled = false;          // the handle serves host-boundary steps / resets through the resident kernel
    bool running = false;          // a resident kernel is (or may still be) on the stream
    uint64_t seq = 0;              // sequence number of the last command posted
};

// the graph-replay rollout (step_graph.hip): the captured graphs, made on the first capture and gone with drop_graphs
struct GraphCache;
struct StepGraphs {
    GraphCache *cache = nullptr;
    int mode = -1;                 // gymnet_launch_policy.graph: -1 = by batch size, 0 = eager launches, 1 = hipGraph replay
};

// the fused rollout's segmented episode records + shard counters (rollout_fused.hip): allocated on first use, grown on demand
struct EpisodeBlock {
    void *d = nullptr;
    EpisodeSegments seg;           // its layout (rollout_plan.hpp)
};

struct RenderStaging;
struct PixelStack;
struct EpisodeMemory;
struct Actor;

}  // namespace gymnet

struct gymnet_vecenv {
    gymnet_config cfg{};
    const gymnet::EnvDesc *desc = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int64_t n = 0, padded = 0, sstride = 0, ostride = 0;
    bool autoreset = false, extras = false;
    // The STATE SCALAR of the handle: float, or double with GYMNET_FLAG_F64 (CartPole only: the reference's own arithmetic,
    // CartPoleEnv.cs:141-166,185).  Every buffer that holds state or observation values — d_state / d_obs and their double-buffer
    // twins, the row-major staging, terminal observations and their compact records, the host-mapped observation staging — holds
    // elements of that type; they are kept as void* here and typed where they are used (esz = element size in bytes).
    bool f64 = false;
    size_t esz = 4;
    // the env's kernel launchers for that state scalar (kernels.hpp EnvLaunchers, found at create; the other pointer stays NULL)
    const gymnet::EnvLaunchers<float> *launch_f32 = nullptr;
    const gymnet::EnvLaunchers<double> *launch_f64 = nullptr;
    // d_state / d_obs always point at the CURRENT (most recently written) buffers; with GYMNET_FLAG_DOUBLE_BUFFER
    // d_state_alt / d_obs_alt are what the next step writes, and the pairs swap after every step launch.
    void *d_state = nullptr, *d_obs = nullptr;
    void *d_state_alt = nullptr, *d_obs_alt = nullptr;
    bool double_buffer = false;
    int cur = 0;                   // index of the buffer d_obs points at (0 = the one reset first wrote)
    float *d_reward = nullptr;
    uint8_t *d_done = nullptr, *d_mask = nullptr;
    int32_t *d_sbd = nullptr;
    uint64_t *d_tick2 = nullptr;
    void *d_actions = nullptr;     // staging for host-path / broadcast actions   (allocated on first use)
    void *d_pack = nullptr;        // row-major obs staging                       (allocated on first use)
    void *d_final_obs = nullptr;
    int32_t *d_done_list = nullptr, *d_done_compact = nullptr;    // sharded segments / compact list (on demand)
    uint32_t *d_done_count2 = nullptr, *d_done_total = nullptr;
    int64_t done_cap = 0;
    float *d_ep_ret = nullptr, *d_fin_ret = nullptr;
    int32_t *d_ep_len = nullptr, *d_fin_len = nullptr;
    // compact per-step records beside the sharded done list (DONE_LIST + EPISODE_STATS / FINAL_OBS), and their gathered copies
    float *d_rec_ret = nullptr, *d_rec_ret_c = nullptr;
    void *d_rec_obs = nullptr, *d_rec_obs_c = nullptr;
    int32_t *d_rec_len = nullptr, *d_rec_len_c = nullptr;
    uint64_t *d_lane_seed = nullptr;       // active per-lane keys (NULL = one key for all lanes)
    uint64_t *d_lane_seed_buf = nullptr;   // the one allocation Seed(int[]) reuses
    unsigned long long *d_after_done = nullptr;
    // small batches (n <= kSmallHostPath): host-mapped staging, so a host-boundary step is 2 kernel launches + 1 sync
    void *hm_actions = nullptr;    // pinned + mapped: the step kernel reads the actions straight from it
    void *hm_obs = nullptr;
    float *hm_reward = nullptr;
    uint8_t *hm_done = nullptr;
    void *hm_block = nullptr;
    // gymnet_vecenv_host_buffers: library-owned page-locked, device-mapped host buffers for the host-boundary path (any batch
    // size); the step's export kernel writes results straight into them, actions are DMA'd out of them
    void *pin_block = nullptr, *pin_actions = nullptr;
    void *pin_obs = nullptr;
    float *pin_reward = nullptr;
    uint8_t *pin_done = nullptr;
    uint32_t *d_bad = nullptr;
    gymnet::Resident res;
    gymnet::EpisodeBlock ep;
    // the four attachments (render.hip, pixel_stack.hip, episode_memory.hip, actor.hip): each unit defines its own type, creates it on
    // config / first use and frees it in its release function below; NULL: none configured
    gymnet::RenderStaging *render = nullptr;
    gymnet::PixelStack *stack = nullptr;
    gymnet::EpisodeMemory *memory = nullptr;
    gymnet::Actor *actor = nullptr;
    uint64_t seed = 0, tick = 0, lane_steps = 0, step_launches = 0;
    uint64_t held_ticks = 0;       // engine ticks that repeated a decision's action (frame skip: R - 1 per decision), see StepMark
    uint64_t obs_epoch = 0;        // entered calls that changed observations, keys or the tick outside a step launch (touch_epoch), see StepMark
    int tslot = 0;                 // which half of d_tick2 the NEXT launch reads (it writes the other half)
    int last_cparity = -1;
    bool async_pending = false;
    std::atomic<bool> busy{false};
    int simds = 1024;              // SIMD units of the device (multiProcessorCount x 4), read at create
    gymnet::LaunchCfg lcfg{4, 256, 0, 0, 1};
    bool can_vec4 = false, can_vec2 = false, lds_ok = false;   // what the buffers' alignment / the batch size allow (set at create)
    bool compact_only = false;     // GYMNET_FLAG_COMPACT_RECORDS_ONLY
    gymnet::StepGraphs graph;
    std::vector<void *> owned;     // device allocations to free
    std::string err;
};

namespace gymnet {

// sets the thread-local last-error message (and the handle's), returns `status`
int fail(gymnet_vecenv *h, int status, const char *fmt, ...);
void set_last_error(const char *msg);

// Restores the caller's current HIP device when it goes out of scope (a process that holds handles on several GPUs —
// or shares the runtime with torch — must not find its current device changed by a library call).
struct DeviceScope {
    int prev = -1;
    DeviceScope() { if (hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipGetLastError(); } }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

struct BusyGuard {
    gymnet_vecenv *h;
    bool ok;
    explicit BusyGuard(gymnet_vecenv *hh) : h(hh), ok(false) {
        bool expect = false;
        ok = h->busy.compare_exchange_strong(expect, true);
    }
    ~BusyGuard() { if (ok) h->busy.store(false); }
};

#define HIP_TRY(h, expr)                                                                              \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return ::gymnet::fail(h, e_ == hipErrorOutOfMemory ? GYMNET_ERR_OOM : GYMNET_ERR_HIP, "%s failed: %s", #expr, \
                                  hipGetErrorString(e_));                                             \
    } while (0)

#define ST_TRY(expr)                  \
    do {                              \
        int s_ = (expr);              \
        if (s_ != GYMNET_OK) return s_; \
    } while (0)

// Entry-point prologue: null check, single-caller guard, switch to the handle's device (restored on return).
// ENTER_KEEP_RESIDENT: the entry points the resident kernel itself serves (host-boundary step / reset).  ENTER: everything else —
// a running resident kernel is told to leave first (it owns the stream and the tick until it has), see resident_stop.
#define ENTER_KEEP_RESIDENT(h)                                                                                     \
    if (!(h)) return ::gymnet::fail(nullptr, GYMNET_ERR_INVALID_ARG, "null handle");                                \
    ::gymnet::BusyGuard guard_(h);                                                                                 \
    if (!guard_.ok) return ::gymnet::fail(h, GYMNET_ERR_ALREADY_STEPPING, "handle is in use by another call");      \
    ::gymnet::DeviceScope dev_scope_;                                                                              \
    (void)hipGetLastError();   /* a stale error left on this thread by anyone must not fail this call's launches */ \
    HIP_TRY(h, hipSetDevice((h)->device))
#define ENTER(h)                                                                                                   \
    ENTER_KEEP_RESIDENT(h);                                                                                        \
    if ((h)->res.running) { int rs_ = ::gymnet::resident_stop(h); if (rs_ != GYMNET_OK) return rs_; }

// Nothing may throw across the C ABI: every entry point body runs inside this guard.
template <class F>
int guarded(F &&f) noexcept {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        set_last_error("host allocation failed (std::bad_alloc)");
        return GYMNET_ERR_OOM;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return GYMNET_ERR_HIP;
    } catch (...) {
        set_last_error("unexpected C++ exception inside the library");
        return GYMNET_ERR_HIP;
    }
}

// The device allocations of one attachment.  A (re-)config take()s everything the new attachment needs into a fresh owner, and only then
// release()s the old one — so a failed re-config leaves the previous attachment working, and an owner that goes out of scope before it was
// installed frees what it took.
struct DeviceAllocs {
    std::vector<void *> ptrs;
    DeviceAllocs() = default;
    DeviceAllocs(const DeviceAllocs &) = delete; DeviceAllocs &operator=(const DeviceAllocs &) = delete;     // (the destructor frees)
    ~DeviceAllocs() { for (void *p : ptrs) (void)hipFree(p); }
    // NULL: out of memory (nothing is reported yet; the caller words the error)
    void *take(size_t bytes) {
        void *p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        ptrs.push_back(p);
        return p;
    }
    // frees everything, after the handle's stream has drained once (a launch may still use it)
    int release(gymnet_vecenv *h) {
        if (!ptrs.empty()) HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (void *p : ptrs) (void)hipFree(p);
        ptrs.clear();
        return GYMNET_OK;
    }
};

// drops the attachment in `slot` (a struct with a DeviceAllocs `mem`); its unit's release function is this, instantiated for its type
template <class A>
int release_attachment(gymnet_vecenv *h, A *&slot) {
    if (!slot) return GYMNET_OK;
    ST_TRY(slot->mem.release(h));
    delete slot;
    slot = nullptr;
    return GYMNET_OK;
}
int release_render(gymnet_vecenv *h), release_stack(gymnet_vecenv *h);      // render.hip, pixel_stack.hip
int release_memory(gymnet_vecenv *h), release_actor(gymnet_vecenv *h);      // episode_memory.hip, actor.hip

// Where the handle's step counters stood at an attachment's last config / reset / push: "exactly one decision since" is
// since(h, m) == {1, 1}, "none" is {0, 0}.  A decision is one vector step, or one action held for R sub-steps in one launch
// (action_repeat.hip): the tick counts DECISION ticks here — engine ticks less h->held_ticks, the R - 1 ticks per decision a frame-skip
// launch holds its action for — so a fused rollout of R steps still reads {R, 1} and T > 1 held decisions read {T, 1}.
// The tick and the launch count alone can be brought back to a marked position (seed rewinds the tick to 0 and a reset adds one; set_tick
// stores any value; set_state moves neither), so the mark also carries h->obs_epoch, which only grows: every entered call that changes
// observations, keys or the tick outside a step launch bumps it (touch_epoch), and since() of a mark taken before such a call has
// epoch != 0 — equal to neither {1, 1} nor {0, 0}, so every gate refuses until the attachment is reset.
struct StepMark { uint64_t tick = 0, launches = 0, epoch = 0; };
inline StepMark mark(const gymnet_vecenv *h) { return {h->tick - h->held_ticks, h->step_launches, h->obs_epoch}; }
inline StepMark since(const gymnet_vecenv *h, StepMark m) {
    return {h->tick - h->held_ticks - m.tick, h->step_launches - m.launches, h->obs_epoch - m.epoch};
}
inline bool operator==(StepMark a, StepMark b) { return a.tick == b.tick && a.launches == b.launches && a.epoch == b.epoch; }
// a reset launch, seed, seed_lanes, set_tick, set_state, per-lane keys installed by set_array: the attachments' marks are void
inline void touch_epoch(gymnet_vecenv *h) { h->obs_epoch += 1; }

// the handle's launcher table, for code typed by its state scalar R
template <class R>
inline const EnvLaunchers<R> &launchers(const gymnet_vecenv *h) {
    if constexpr (sizeof(R) == 8) return *h->launch_f64; else return *h->launch_f32;
}

// address of row k of a [rows][stride] structure-of-arrays buffer of esz-byte elements
inline void *row_at(void *base, int64_t k, int64_t stride, size_t esz) { return static_cast<char *>(base) + (size_t)k * (size_t)stride * esz; }
// bytes one env-step of this handle moves by the algorithmic count: 41 for float32 CartPole, 73 in float64
// (32 B state read + 4 B action + 32 B state written + 4 B reward + 1 B done)
inline size_t bytes_per_step(const gymnet_vecenv *h) { return h->f64 ? (size_t)73 : (size_t)h->desc->algorithmic_bytes; }

// (aligned16, aligned_to: rollout_plan.hpp)

// the arguments of a step launch that reads its actions at d_actions / of a reset of the lanes d_mask marks (NULL = all lanes), as the
// handle stands
template <class R>
inline StepArgsT<R> make_step_args(gymnet_vecenv *h, const void *d_actions) {
    StepArgsT<R> a{};
    const bool alias = h->desc->alias;
    a.state = static_cast<R *>(h->d_state);
    a.state_out = static_cast<R *>((h->double_buffer && alias) ? h->d_state_alt : h->d_state);
    a.obs = static_cast<R *>((h->double_buffer && !alias) ? h->d_obs_alt : h->d_obs);
    a.obs_in = static_cast<const R *>(h->d_obs);
    a.action = d_actions;
    a.reward = h->d_reward;
    a.done = h->d_done;
    a.sbd = h->d_sbd;
    a.tick2 = h->d_tick2;
    // the dense "last finished episode per lane" arrays are maintained by the step kernel itself unless the caller opted for
    // compact records only (GYMNET_FLAG_COMPACT_RECORDS_ONLY with DONE_LIST): then the getters apply the records on demand
    const bool dense = !(h->compact_only && h->d_done_list);
    a.final_obs = dense ? static_cast<R *>(h->d_final_obs) : nullptr;
    a.done_list = h->d_done_list;
    a.done_count2 = h->d_done_count2;
    a.done_cap = h->done_cap;
    a.ep_ret = h->d_ep_ret; a.ep_len = h->d_ep_len; a.fin_ret = dense ? h->d_fin_ret : nullptr; a.fin_len = dense ? h->d_fin_len : nullptr;
    a.rec_ret = h->d_rec_ret; a.rec_len = h->d_rec_len; a.rec_obs = static_cast<R *>(h->d_rec_obs);
    a.lane_seed = h->d_lane_seed;
    a.after_done = h->d_after_done;
    a.n = h->n; a.state_stride = h->sstride; a.obs_stride = h->ostride;
    a.lane_offset = (uint64_t)h->cfg.lane_offset;
    a.seed = h->seed;
    a.parity = (int32_t)h->tslot;
    a.cparity = (int32_t)(h->step_launches & 1u);
    a.max_episode_steps = h->cfg.max_episode_steps;
    return a;
}
template <class R>
inline ResetArgsT<R> make_reset_args(gymnet_vecenv *h, const uint8_t *d_mask) {
    ResetArgsT<R> r{};
    r.state = static_cast<R *>(h->d_state); r.obs = static_cast<R *>(h->d_obs); r.sbd = h->d_sbd; r.done = h->d_done;
    r.mask = d_mask;
    r.tick2 = h->d_tick2; r.lane_seed = h->d_lane_seed;
    r.ep_ret = h->d_ep_ret; r.ep_len = h->d_ep_len;
    r.n = h->n; r.state_stride = h->sstride; r.obs_stride = h->ostride;
    r.lane_offset = (uint64_t)h->cfg.lane_offset; r.seed = h->seed;
    r.parity = (int32_t)h->tslot;
    return r;
}

// ---- helpers that assume the caller already ENTERed the handle (device set, busy flag held) ----------------------
// Discrete.Contains over `slices` device slices of h->n actions each, slice k at slice_of(k), with one readback; blocks.  *bad: how many
// actions lie outside the space (the callers word the error: lanes of one batch, lane-steps of a rollout)
template <class SliceOf>
inline int count_bad_actions(gymnet_vecenv *h, int64_t slices, SliceOf slice_of, uint32_t *bad) {
    HIP_TRY(h, hipMemsetAsync(h->d_bad, 0, sizeof(uint32_t), h->stream));
    for (int64_t k = 0; k < slices; ++k)
        HIP_TRY(h, launch_validate_discrete(static_cast<const int32_t *>(slice_of(k)), h->n, h->desc->action_n, h->d_bad, h->stream));
    *bad = 0;
    HIP_TRY(h, hipMemcpyAsync(bad, h->d_bad, sizeof *bad, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GYMNET_OK;
}
// capi.hip
int launch_one_step(gymnet_vecenv *h, const void *d_actions);       // one vector step = one kernel launch
int launch_reset_lanes(gymnet_vecenv *h, const uint8_t *d_mask);    // NULL = all lanes
void swap_buffers(gymnet_vecenv *h);                                 // after a step launch with GYMNET_FLAG_DOUBLE_BUFFER: what was written becomes current
int stage_host_actions(gymnet_vecenv *h, const void *actions, const void **d_use, bool validate_now);
int validate_staged_actions(gymnet_vecenv *h, const void *d_actions);
// obs_out: float32 [n, obs_dim], or float64 for a GYMNET_FLAG_F64 handle
int queue_copy_out(gymnet_vecenv *h, void *obs_out, float *reward_out, uint8_t *done_out);   // no final sync (large-batch path)
int copy_out(gymnet_vecenv *h, void *obs_out, float *reward_out, uint8_t *done_out);         // blocks
int write_tick(gymnet_vecenv *h);
int seed_handle(gymnet_vecenv *h, uint64_t seed);                    // Env.Seed(int): new key, tick 0, captured graphs dropped
// launch_policy.hip
void default_policy(gymnet_vecenv *h);                               // the launch configuration a handle starts with (launch_policy.hpp), at create
// step_graph.hip
// graph_mode: -1 = by batch size (replay only while launch-bound), 0 = eager launches, 1 = always replay a captured graph
int rollout_steps(gymnet_vecenv *h, const void *d_actions, int64_t steps, int64_t action_stride, int64_t ring, int graph_mode = -1);
void drop_graphs(gymnet_vecenv *h);                                  // whatever a captured launch froze (configuration, seed, keys) changes
// resident.hip
int resident_create(gymnet_vecenv *h);                               // the mailbox of a GYMNET_FLAG_RESIDENT handle, at create
void resident_release(gymnet_vecenv *h);                             // stops the kernel and frees the mailbox, at destroy
int resident_stop(gymnet_vecenv *h);                                 // tells a running resident kernel to leave and waits until it has
bool resident_serves(const gymnet_vecenv *h);                        // the resident path serves this handle's host-boundary steps right now
// one command (kMailboxStep / ResetAll / ResetDone) through the mailbox: post it, wait for its results, copy them out
int resident_command(gymnet_vecenv *h, uint32_t cmd, const void *actions, void *obs_out, float *reward_out, uint8_t *done_out);
// rollout_fused.hip
// gymnet_vecenv_rollout_fused_ex_device on a handle the caller has ENTERed (rollout_plan.hpp FusedRequest: the spec, frame skip, the
// record pointers of the logp / value calls): gather the facts, plan or refuse, allocate and launch, move the ticks
int rollout_fused_entered(gymnet_vecenv *h, const FusedRequest &rq);
// the fused rollout with GYMNET_ACTIONS_ACTOR (actor.hip): what the plan reads of the handle's actor; the launch, by the unit that serves
// the handle as it stands (records: the rollout keeps compact episode records; rq.rec_logp / rq.rec_value: where it records every step's
// log-probability / critic value, [steps][n], null: nowhere); afterwards the history's newest slot has moved `steps` on and is current
ActorFacts actor_facts(const gymnet_vecenv *h);
hipError_t actor_rollout_launch(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r, const FusedRequest &rq);
void actor_rollout_done(gymnet_vecenv *h, int64_t steps);
// the fused rollout with frame skip (action_repeat.hip): r.steps decisions of R sub-steps each under one action, one launch
hipError_t repeat_rollout_launch(gymnet_vecenv *h, const StepArgs &a, const RolloutArgs &r, int32_t R);
hipError_t repeat_rollout_launch(gymnet_vecenv *h, const StepArgs64 &a, const RolloutArgs64 &r, int32_t R);

}  // namespace gymnet
