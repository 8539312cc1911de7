// rollout_plan.hpp — what a fused rollout call will do, as a pure function of plain values: every refusal (status and text, in the order
// the calls have always reported them), the lane width the rollout kernel is launched with, the episode-segment block it needs, the ticks
// it moves.  Host only: no HIP header, so tests/cpp/rollout_plan_test.cpp holds every rule from both sides on a CPU (g++ -std=c++17).
// rollout_fused.hip gathers the facts from a handle, calls the plan, allocates, launches and applies the ticks; kernels.hpp includes this
// for kShards / kCountStride.  Pointers are read for being null and for their alignment only; nothing here follows one (but the spec's).
#pragma once
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/gymnet_amd.h"

namespace gymnet {

constexpr int kShards = 256;        // power of two; the gather kernels' workgroup size (kernels.hip static_assert)
constexpr int kCountStride = 16;    // uint32 words between shard counters (64 bytes: one counter per cache line)

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned_to(const void *p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) == 0; }

// The segment block of the fused rollout's episode records: four arrays (t, lane, return, length) of [kShards segments of `cap` records |
// one overflow segment of `ov_cap` records] each, then kShards + 1 counters (a cache line each).  Random lanes do not fill the shards evenly,
// so a segment gets twice its share of the caller's capacity — and what a shard still cannot hold (lanes that finish very unevenly) goes to
// ONE shared overflow segment of `capacity` records (round 6): records are dropped only when more episodes end than the
// caller's arrays hold.
struct EpisodeSegments {
    int64_t cap = 0;               // records per shard segment
    int64_t ov_cap = 0;            // records of the shared overflow segment (= the largest ep_capacity asked for so far)
    // the segment capacity a caller's ep_capacity asks for
    static int64_t cap_for(int64_t capacity) { return 2 * ((capacity + kShards - 1) / kShards) + 64; }
    bool holds(int64_t capacity) const { return cap_for(capacity) <= cap && capacity <= ov_cap; }
    size_t array_bytes() const { return ((size_t)kShards * (size_t)cap + (size_t)ov_cap) * 4; }
    size_t offset(int array) const { return (size_t)array * array_bytes(); }      // 0: t, 1: lane, 2: return, 3: length
    size_t counters_offset() const { return 4 * array_bytes(); }
    size_t bytes() const { return ((size_t)kShards * (size_t)cap + (size_t)ov_cap) * 16 + (size_t)(kShards + 1) * kCountStride * 4 + 8; }
};

// What the plan reads of a handle.
enum class ActorKind { None, Discrete, Box };
struct ActorFacts {
    ActorKind kind = ActorKind::None;
    bool critic = false;           // a critic is configured (actor_value.hip)
    bool current = false;          // the history is current: no vector step since the last actor config, reset, push or actor rollout
    float box_sigma = 0;           // a Box actor's policy's sigma (gymnet_vecenv_actor_box_set_policy)
};
struct FusedFacts {
    int64_t n = 0, sstride = 0;
    bool f64 = false, alias = false, box_action = false;      // the state scalar; EnvDesc::alias, EnvDesc::box_action
    bool extras = false;           // a bookkeeping handle (EPISODE_STATS / DONE_LIST / FINAL_OBS, or per-lane seeds)
    bool ep_stats = false;         // episode statistics exist (d_ep_ret)
    bool validate_actions = false; // GYMNET_FLAG_VALIDATE_ACTIONS
    int vec = 1;                   // h->lcfg.vec
    ActorFacts actor;
    bool has_segments = false;     // a segment block is allocated, of ...
    EpisodeSegments segments;      // ... these capacities
    int32_t max_episode_steps = 0; // the handle's time limit (0: none; > 0 implies EPISODE_STATS, so a bookkeeping handle)
};

// What the caller asked for; also the one argument the rollout's host code hands down to the launch (actor_rollout_launch reads the two
// record pointers).  spec: gymnet_vecenv_rollout_fused_ex_device's, as given (null and a wrong struct_size are the plan's to refuse).
// held: frame skip — spec.steps decisions of held + 1 sub-steps each (action_repeat.hip); 0: the fused rollout.  validated: the caller has
// run VALIDATE_ACTIONS over the one slice read (gymnet_vecenv_step_repeat_device).  rec_logp / rec_value: where an actor rollout records
// every step's log-probability / critic value (gymnet_vecenv_rollout_fused_logp_device, _value_device; null: nowhere).  rec_logd: where a
// Box actor's rollout records every step's log-density, and box_value: rec_value is that call's (gymnet_vecenv_rollout_fused_box_logd_device
// alone sets it, so that rec_value without rec_logd reaches a Box actor there and nowhere else; the _box_boot_ call sets it whenever it
// has a boot pointer).  rec_boot: where an actor rollout records every step's V(terminal observation) on time-limit rows
// (gymnet_vecenv_rollout_fused_value_boot_device, _box_boot_device, actor_boot.hip; null: nowhere)
struct FusedRequest {
    const gymnet_rollout_spec *spec = nullptr;
    int32_t held = 0;
    bool validated = false;
    float *rec_logp = nullptr, *rec_value = nullptr;
    float *rec_logd = nullptr;
    bool box_value = false;
    float *rec_boot = nullptr;
};

struct FusedPlan {
    bool ring_read = false;        // the kernel reads d_actions (RING, EPSILON_GREEDY)
    bool actor = false;            // GYMNET_ACTIONS_ACTOR
    bool episodes = false;         // the rollout keeps compact episode records
    bool zero_steps = false;       // steps == 0: nothing is launched (d_ep_count is zeroed where episodes), no tick moves
    int vec = 1;                   // lanes per thread of the rollout kernel
    EpisodeSegments segments;      // episodes: the block the launch runs on ...
    bool grow = false;             // ... which must be allocated first: the handle's is missing or smaller
    int64_t ov_cap = 0;            // episodes: records of the overflow segment this rollout may fill
    uint64_t ticks = 0;            // engine ticks the launch moves (a sub-step is an engine tick) ...
    uint64_t held_ticks = 0;       // ... and how many of them repeated a decision's action
};
// status GYMNET_OK: plan holds; else the refusal, text as gymnet_last_error reports it
struct FusedOutcome { int status = GYMNET_OK; FusedPlan plan; char text[512]; };

// the actor refusals the rollout shares with the act / push / view calls (actor_net.hpp need_actor) and words itself
constexpr char kNoActorFormat[] = "no actor configured (%s)";
inline const char *actor_config_call(bool box_action) { return box_action ? "gymnet_vecenv_actor_box_config" : "gymnet_vecenv_actor_config"; }
constexpr char kStaleForRollout[] = "the actor's history is stale: reset the actor (or push) before an actor rollout";

// The Box actor's log-density (actor_box_logd.hip): what the kernels take of sigma, computed in float64 and rounded once, and the sigmas
// it is defined for: > 0 with a finite float32 reciprocal
struct BoxLogd { float inv_sigma, c; };
inline bool box_sigma_ok(float sigma) { return sigma > 0.0f && std::isfinite(1.0f / sigma); }
inline BoxLogd box_logd_args(float sigma) {
    return {(float)(1.0 / (double)sigma), (float)(-std::log((double)sigma) - 0.91893853320467274178)};     // -ln sigma - ln(2 pi) / 2
}
constexpr char kBadSigmaFormat[] = "%s: the log-density needs a policy with sigma > 0 and a finite 1 / sigma (gymnet_vecenv_actor_box_set_policy), not %g";

namespace plan_detail {

__attribute__((format(printf, 3, 4))) inline int refuse(char (&text)[512], int status, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    return status;
}

// gymnet_vecenv_rollout_fused_logp_device's checks of its record pointer (the source, the actor's kind, the alignment) and
// gymnet_vecenv_rollout_fused_value_device's of its two (the same, and that the Discrete actor has a critic), which run before the
// rollout's own.  A value pointer makes it the value call: the logp call forwards there only without one.  A boot pointer
// (gymnet_vecenv_rollout_fused_value_boot_device) needs the value pointer — asked first, it says which call this is —, then every check of
// the value call applies in its order, then the boot's own: a time limit, the alignment
constexpr char kBootNeedsValue[] = "d_rec_boot: V(terminal observation) is recorded beside the values: d_rec_value is null";
constexpr char kBootNeedsLimit[] = "d_rec_boot: this handle has no time limit (max_episode_steps == 0): no episode is truncated and no row needs a boot";
inline int boot_pointer(const FusedFacts &f, const FusedRequest &rq, char (&text)[512]) {
    if (!rq.rec_boot) return GYMNET_OK;
    if (f.max_episode_steps <= 0) return refuse(text, GYMNET_ERR_INVALID_ARG, "%s", kBootNeedsLimit);
    if (!aligned_to(rq.rec_boot, 4)) return refuse(text, GYMNET_ERR_INVALID_ARG, "d_rec_boot must be 4-byte aligned");
    return GYMNET_OK;
}
inline int record_pointers(const FusedFacts &f, const FusedRequest &rq, int32_t action_source, char (&text)[512]) {
    const bool value = rq.rec_value != nullptr;
    if (rq.rec_boot && !value) return refuse(text, GYMNET_ERR_INVALID_ARG, "%s", kBootNeedsValue);
    if (action_source != GYMNET_ACTIONS_ACTOR)
        return value ? refuse(text, GYMNET_ERR_INVALID_ARG, "d_rec_value: values are recorded where the actor chooses (action_source GYMNET_ACTIONS_ACTOR), not %d", action_source)
                     : refuse(text, GYMNET_ERR_INVALID_ARG, "d_rec_logp: log-probabilities are recorded where the actor chooses (action_source GYMNET_ACTIONS_ACTOR), not %d", action_source);
    if (f.actor.kind == ActorKind::None) return refuse(text, GYMNET_ERR_INVALID_ARG, kNoActorFormat, actor_config_call(f.box_action));
    if (f.actor.kind == ActorKind::Box)
        return value ? refuse(text, GYMNET_ERR_INVALID_ARG, "d_rec_value: this handle's actor chooses Box actions; the fused rollout records values for a Discrete actor "
                              "(gymnet_vecenv_actor_value_device serves a Box actor)")
                     : refuse(text, GYMNET_ERR_INVALID_ARG, "d_rec_logp: this handle's actor chooses Box actions; a log-probability belongs to a Discrete actor");
    if (value && !f.actor.critic) return refuse(text, GYMNET_ERR_INVALID_ARG, "d_rec_value: no critic configured (gymnet_vecenv_actor_critic_config)");
    if (!aligned_to(rq.rec_logp, 4)) return refuse(text, GYMNET_ERR_INVALID_ARG, "d_rec_logp must be 4-byte aligned");
    if (value && !aligned_to(rq.rec_value, 4)) return refuse(text, GYMNET_ERR_INVALID_ARG, "d_rec_value must be 4-byte aligned");
    return boot_pointer(f, rq, text);
}

// gymnet_vecenv_rollout_fused_box_logd_device's checks of its two record pointers, which run before the rollout's own: the source, an
// actor, its kind, its sigma, a critic where values are asked for, the alignments; with a boot pointer
// (gymnet_vecenv_rollout_fused_box_boot_device) around them what record_pointers puts around its own
inline int box_record_pointers(const FusedFacts &f, const FusedRequest &rq, int32_t action_source, char (&text)[512]) {
    const char *what = rq.rec_logd ? "d_rec_logd" : "d_rec_value";
    const bool value = rq.box_value && rq.rec_value != nullptr;
    if (rq.rec_boot && !value) return refuse(text, GYMNET_ERR_INVALID_ARG, "%s", kBootNeedsValue);
    if (action_source != GYMNET_ACTIONS_ACTOR)
        return refuse(text, GYMNET_ERR_INVALID_ARG, "%s: log-densities and values are recorded where the actor chooses (action_source GYMNET_ACTIONS_ACTOR), not %d", what, action_source);
    if (f.actor.kind == ActorKind::None) return refuse(text, GYMNET_ERR_INVALID_ARG, kNoActorFormat, actor_config_call(f.box_action));
    if (f.actor.kind == ActorKind::Discrete)
        return refuse(text, GYMNET_ERR_INVALID_ARG, "%s: this handle's actor chooses Discrete actions; a log-density belongs to a Box actor "
                      "(gymnet_vecenv_rollout_fused_value_device records a Discrete actor's log-probability and value)", what);
    if (!box_sigma_ok(f.actor.box_sigma)) return refuse(text, GYMNET_ERR_INVALID_ARG, kBadSigmaFormat, what, (double)f.actor.box_sigma);
    if (value && !f.actor.critic) return refuse(text, GYMNET_ERR_INVALID_ARG, "d_rec_value: no critic configured (gymnet_vecenv_actor_critic_config)");
    if (!aligned_to(rq.rec_logd, 4)) return refuse(text, GYMNET_ERR_INVALID_ARG, "d_rec_logd must be 4-byte aligned");
    if (value && !aligned_to(rq.rec_value, 4)) return refuse(text, GYMNET_ERR_INVALID_ARG, "d_rec_value must be 4-byte aligned");
    return boot_pointer(f, rq, text);
}

inline int plan(const FusedFacts &f, const FusedRequest &rq, FusedPlan &p, char (&text)[512]) {
    const int32_t held = rq.held;
    if (!rq.spec) return refuse(text, GYMNET_ERR_INVALID_ARG, "spec is null");
    if (rq.spec->struct_size != sizeof(gymnet_rollout_spec))
        return refuse(text, GYMNET_ERR_INVALID_ARG, "spec.struct_size %u != %zu (ABI mismatch)", rq.spec->struct_size, sizeof(gymnet_rollout_spec));
    const gymnet_rollout_spec &sp = *rq.spec;
    if (rq.rec_logd || rq.box_value) {
        const int s = box_record_pointers(f, rq, sp.action_source, text);
        if (s != GYMNET_OK) return s;
    } else if (rq.rec_logp || rq.rec_value || rq.rec_boot) {
        const int s = record_pointers(f, rq, sp.action_source, text);
        if (s != GYMNET_OK) return s;
    }
    if (sp.action_source < GYMNET_ACTIONS_RING || sp.action_source > GYMNET_ACTIONS_ACTOR) return refuse(text, GYMNET_ERR_INVALID_ARG, "bad action_source %d", sp.action_source);
    const bool actor = sp.action_source == GYMNET_ACTIONS_ACTOR;
    const bool ring_read = sp.action_source != GYMNET_ACTIONS_SAMPLE && !actor;
    if (ring_read && !sp.d_actions) return refuse(text, GYMNET_ERR_INVALID_ARG, "d_actions is null");
    if (sp.steps < 0 || (ring_read && (sp.ring < 1 || sp.action_stride < 0))) return refuse(text, GYMNET_ERR_INVALID_ARG, "bad steps/ring/action_stride");
    if (sp.steps > INT32_MAX) return refuse(text, GYMNET_ERR_INVALID_ARG, "steps must fit an int32 (episode records carry the step index)");
    // ABI 5 called this field `reserved`: a caller that left it uninitialised must not select the lossy no-overflow variant by accident
    if (sp.record_flags & ~GYMNET_RECORDS_NO_OVERFLOW) return refuse(text, GYMNET_ERR_INVALID_ARG, "unknown record_flags bits 0x%x", (unsigned)sp.record_flags);
    if (sp.action_source == GYMNET_ACTIONS_EPSILON_GREEDY) {
        if (f.box_action) return refuse(text, GYMNET_ERR_UNSUPPORTED, "epsilon-greedy composition is defined for Discrete action spaces");
        if (!(sp.epsilon >= 0.0f && sp.epsilon <= 1.0f)) return refuse(text, GYMNET_ERR_INVALID_ARG, "epsilon must be in [0, 1]");
    }
    if (actor && held > 0)
        return refuse(text, GYMNET_ERR_UNSUPPORTED, "the fused actor rollout has no frame skip: run the unfused loop, one decision at a time "
                      "(actor_act_device, step_repeat_device, actor_push_device)");
    if (held > 0 && sp.steps * ((int64_t)held + 1) > INT32_MAX)
        return refuse(text, GYMNET_ERR_INVALID_ARG, "steps * (repeat + 1) must fit an int32");
    if (actor) {
        if (f.f64) return refuse(text, GYMNET_ERR_UNSUPPORTED, "the fused actor rollout runs float32 handles (float64: act / step / push)");
        if (!(sp.epsilon >= 0.0f && sp.epsilon <= 1.0f)) return refuse(text, GYMNET_ERR_INVALID_ARG, "epsilon must be in [0, 1]");
        // may it run: an actor is configured and its history is current
        if (f.actor.kind == ActorKind::None) return refuse(text, GYMNET_ERR_INVALID_ARG, kNoActorFormat, actor_config_call(f.box_action));
        if (!f.actor.current) return refuse(text, GYMNET_ERR_INVALID_ARG, "%s", kStaleForRollout);
    }
    if (f.validate_actions && ring_read && !rq.validated)
        return refuse(text, GYMNET_ERR_UNSUPPORTED, "VALIDATE_ACTIONS is per step; use gymnet_vecenv_rollout_device (sampled actions are valid by construction)");
    const bool episodes = sp.d_ep_lane || sp.d_ep_step || sp.d_ep_return || sp.d_ep_length || sp.d_ep_count;
    if (episodes) {
        if (!f.extras) return refuse(text, GYMNET_ERR_UNSUPPORTED, "episode records need a bookkeeping handle (GYMNET_FLAG_EPISODE_STATS / DONE_LIST / FINAL_OBS)");
        if ((sp.d_ep_return || sp.d_ep_length) && !f.ep_stats) return refuse(text, GYMNET_ERR_UNSUPPORTED, "episode return / length records need GYMNET_FLAG_EPISODE_STATS");
        if (sp.ep_capacity < 0 || !sp.d_ep_count) return refuse(text, GYMNET_ERR_INVALID_ARG, "episode records need ep_capacity >= 0 and d_ep_count");
    }
    if (sp.d_rec_actions && !f.extras && sp.action_source == GYMNET_ACTIONS_RING)
        return refuse(text, GYMNET_ERR_UNSUPPORTED, "d_rec_actions: the actions of a plain ring rollout ARE the ring (recorded for sampled / epsilon-greedy actions and on bookkeeping handles)");
    p.ring_read = ring_read; p.actor = actor; p.episodes = episodes;
    if (sp.steps == 0) {
        p.zero_steps = true;
        return GYMNET_OK;
    }
    p.vec = f.vec;
    // wide accesses on the streams a rollout touches: 16-byte rows of observations (4 floats / 2 doubles per thread), vec rewards /
    // actions, vec done bytes; anything less aligned runs one lane per thread (same bits)
    if (p.vec > 1) {
        auto streams_fit = [&](int w) {
            bool ok = (f.n % w) == 0;
            if (ring_read) ok = ok && aligned_to(sp.d_actions, 4 * w) && (sp.action_stride % w) == 0;
            return ok && (!sp.d_rec_obs || aligned16(sp.d_rec_obs)) && (!sp.d_rec_reward || aligned_to(sp.d_rec_reward, 4 * w)) &&
                   (!sp.d_rec_done || aligned_to(sp.d_rec_done, w)) && (!sp.d_rec_actions || aligned_to(sp.d_rec_actions, 4 * w));
        };
        const int w = f.f64 ? 2 : p.vec;                  // the fused rollout's wide form: 2 doubles / 4 floats (2: Acrobot) per thread
        // the FAT form where every stream allows it — float64: FOUR lanes per thread (the state sits in registers for the whole rollout, so
        // this is about how many lanes share a wave's per-step overheads, not about access width; launch_rollout_env) — else two, else one;
        // (float32 has no fat form: eight floats per thread were measured slower, step_kernels.hpp rollout_fat_lanes)
        if (f.f64 && f.alias && (f.sstride % 4) == 0 && streams_fit(4)) p.vec = 4;
        else if (!streams_fit(w)) p.vec = 1;
    }
    if (episodes) {
        p.grow = !(f.has_segments && f.segments.holds(sp.ep_capacity));
        p.segments = p.grow ? EpisodeSegments{EpisodeSegments::cap_for(sp.ep_capacity), sp.ep_capacity} : f.segments;
        p.ov_cap = sp.ep_capacity < p.segments.ov_cap ? sp.ep_capacity : p.segments.ov_cap;
    }
    p.ticks = (uint64_t)sp.steps * ((uint64_t)held + 1);       // a sub-step is an engine tick
    p.held_ticks = p.ticks - (uint64_t)sp.steps;
    return GYMNET_OK;
}

}  // namespace plan_detail

inline FusedOutcome plan_fused_rollout(const FusedFacts &f, const FusedRequest &rq) {
    FusedOutcome out;
    out.text[0] = '\0';
    out.status = plan_detail::plan(f, rq, out.plan, out.text);
    return out;
}

}  // namespace gymnet
