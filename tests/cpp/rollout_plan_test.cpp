// rollout_plan_test.cpp — the fused rollout's plan (gym.net_amd/csrc/rollout_plan.hpp), a pure function, held to a table on the CPU:
// every refusal as the first failure and in its order, every lane-width rule from both sides, the episode-segment block.
// g++ -std=c++17, no library, no HIP.  Pointers are integers here: the plan reads their alignment and whether they are null.
//
// Expected values are what rollout_fused_entered and the two record-pointer checks gave as they stood in capi.hip / actor.hip before they
// became this header (their text behind a shim handle in a scratch harness, which ran every row below and compared both over an
// enumerated product: docs/ledger.md §35) — never the code under test.  Each width row was also checked by hand against streams_fit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../gym.net_amd/csrc/rollout_plan.hpp"

using namespace gymnet;

namespace {

static_assert(sizeof(gymnet_rollout_spec) == 144, "the struct_size row below spells 144");

// a 4096-byte aligned address plus `off` bytes, one page per stream
void *at(int stream, int64_t off) { return reinterpret_cast<void *>((uintptr_t)0x7f0000000000ull + (uintptr_t)stream * 0x100000u + (uintptr_t)off); }
enum { ACT = 1, OBS, REW, DONE, RACT, LOGP, VALUE, EP };

// handles: CartPole float32 (alias, Discrete), Acrobot (derived observation, Discrete), float64 CartPole, Pendulum (Box)
FusedFacts cartpole(int64_t n = 1024, int vec = 4) {
    FusedFacts f;
    f.n = n; f.sstride = (n + 63) / 64 * 64; f.alias = true; f.vec = vec;
    return f;
}
FusedFacts acrobot(int64_t n = 1024, int vec = 2) { FusedFacts f = cartpole(n, vec); f.alias = false; return f; }
FusedFacts cartpole64(int64_t n, int vec = 2) { FusedFacts f = cartpole(n, vec); f.f64 = true; return f; }
FusedFacts pendulum(int64_t n = 1024, int vec = 4) { FusedFacts f = cartpole(n, vec); f.alias = false; f.box_action = true; return f; }
FusedFacts bookkeeping(FusedFacts f, bool stats = true) { f.extras = true; f.ep_stats = stats; return f; }
FusedFacts validating(FusedFacts f) { f.validate_actions = true; return f; }
FusedFacts with_actor(FusedFacts f, ActorKind kind, bool current = true, bool critic = false) { f.actor = ActorFacts{kind, critic, current}; return f; }
FusedFacts holding(FusedFacts f, int64_t cap, int64_t ov) { f.has_segments = true; f.segments = EpisodeSegments{cap, ov}; return f; }

// a request: the spec by value (null_spec: the call got none), and the rest of FusedRequest
struct Ask {
    gymnet_rollout_spec sp{};
    bool null_spec = false;
    int32_t held = 0;
    bool validated = false;
    void *rec_logp = nullptr, *rec_value = nullptr;
};
// a ring rollout of 8 steps over n lanes; streams: observation, reward and done recorded, every stream aligned
Ask ring(int64_t n = 1024, bool streams = true) {
    Ask a;
    a.sp.struct_size = sizeof a.sp; a.sp.action_source = GYMNET_ACTIONS_RING;
    a.sp.d_actions = at(ACT, 0); a.sp.steps = 8; a.sp.action_stride = n; a.sp.ring = 1;
    if (streams) { a.sp.d_rec_obs = at(OBS, 0); a.sp.d_rec_reward = static_cast<float *>(at(REW, 0)); a.sp.d_rec_done = static_cast<uint8_t *>(at(DONE, 0)); }
    return a;
}
Ask source(Ask a, int32_t s) { a.sp.action_source = s; return a; }
Ask actions_at(Ask a, int64_t off) { a.sp.d_actions = at(ACT, off); return a; }
Ask no_actions(Ask a) { a.sp.d_actions = nullptr; return a; }
Ask stride(Ask a, int64_t s) { a.sp.action_stride = s; return a; }
Ask obs_at(Ask a, int64_t off) { a.sp.d_rec_obs = at(OBS, off); return a; }
Ask reward_at(Ask a, int64_t off) { a.sp.d_rec_reward = static_cast<float *>(at(REW, off)); return a; }
Ask done_at(Ask a, int64_t off) { a.sp.d_rec_done = static_cast<uint8_t *>(at(DONE, off)); return a; }
Ask rec_actions_at(Ask a, int64_t off) { a.sp.d_rec_actions = at(RACT, off); return a; }
Ask steps(Ask a, int64_t s) { a.sp.steps = s; return a; }
Ask ring_len(Ask a, int64_t r) { a.sp.ring = r; return a; }
Ask flags(Ask a, int32_t fl) { a.sp.record_flags = fl; return a; }
Ask epsilon(Ask a, float e) { a.sp.epsilon = e; return a; }
Ask held(Ask a, int32_t hd, bool validated = false) { a.held = hd; a.validated = validated; return a; }
Ask logp_at(Ask a, int64_t off) { a.rec_logp = at(LOGP, off); return a; }
Ask value_at(Ask a, int64_t off) { a.rec_value = at(VALUE, off); return a; }
Ask null_spec(Ask a) { a.null_spec = true; return a; }
Ask struct_size(Ask a, uint32_t s) { a.sp.struct_size = s; return a; }
// episode records of `capacity`: step, lane and count; with_stats: return and length too; count: d_ep_count given
Ask episodes(Ask a, int64_t capacity, bool with_stats = true, bool count = true) {
    a.sp.d_ep_step = static_cast<int32_t *>(at(EP, 0)); a.sp.d_ep_lane = static_cast<int32_t *>(at(EP, 0x10000));
    if (with_stats) { a.sp.d_ep_return = static_cast<float *>(at(EP, 0x20000)); a.sp.d_ep_length = static_cast<int32_t *>(at(EP, 0x30000)); }
    if (count) a.sp.d_ep_count = static_cast<uint32_t *>(at(EP, 0x40000));
    a.sp.ep_capacity = capacity;
    return a;
}

// what a row expects: a refusal (status, text) or the plan's fields
struct Want {
    int status = GYMNET_OK;
    const char *text = "";
    FusedPlan plan;
};
Want refused(int status, const char *text) { Want w; w.status = status; w.text = text; return w; }
constexpr int ARG = GYMNET_ERR_INVALID_ARG, UNS = GYMNET_ERR_UNSUPPORTED;
// a plan of `vec` lanes per thread for 8 steps read from the ring
Want planned(int vec, uint64_t ticks = 8, uint64_t held_ticks = 0) {
    Want w;
    w.plan.ring_read = true; w.plan.vec = vec; w.plan.ticks = ticks; w.plan.held_ticks = held_ticks;
    return w;
}
Want unread(Want w, bool actor = false) { w.plan.ring_read = false; w.plan.actor = actor; return w; }
Want with_segments(Want w, int64_t cap, int64_t ov, bool grow, int64_t ov_cap) {
    w.plan.episodes = true; w.plan.segments = EpisodeSegments{cap, ov}; w.plan.grow = grow; w.plan.ov_cap = ov_cap;
    return w;
}
Want nothing_to_do(bool episodes, bool ring_read = true) { Want w; w.plan.zero_steps = true; w.plan.episodes = episodes; w.plan.ring_read = ring_read; return w; }

struct Row { const char *name; FusedFacts f; Ask a; Want w; };

const float kBelow0 = std::nextafter(0.0f, -1.0f), kAbove1 = std::nextafter(1.0f, 2.0f), kNaN = std::numeric_limits<float>::quiet_NaN();
const int64_t kMax = INT32_MAX;
const FusedFacts kDiscrete = with_actor(cartpole(), ActorKind::Discrete), kCritic = with_actor(cartpole(), ActorKind::Discrete, true, true);
const FusedFacts kBox = with_actor(pendulum(), ActorKind::Box);
const Ask kActor = source(ring(), GYMNET_ACTIONS_ACTOR);

const std::vector<Row> kRows = {
    // ---- lane width, float32 CartPole with lcfg.vec = 4 (streams_fit(4): n % 4, d_actions 16, stride % 4, obs 16, reward 16, done 4, actions 16)
    {"f32 every stream aligned", cartpole(), ring(), planned(4)},
    {"f32 no stream recorded", cartpole(), ring(1024, false), planned(4)},
    {"f32 n % 4 == 1", cartpole(1025), ring(1025), planned(1)},
    {"f32 n % 4 == 1, stride a multiple of 4", cartpole(1025), stride(ring(1025), 1028), planned(1)},
    {"f32 d_actions 4 bytes off", cartpole(), actions_at(ring(), 4), planned(1)},
    {"f32 d_actions 8 bytes off", cartpole(), actions_at(ring(), 8), planned(1)},
    {"f32 d_actions 12 bytes off", cartpole(), actions_at(ring(), 12), planned(1)},
    {"f32 action_stride % 4 == 1", cartpole(), stride(ring(), 1025), planned(1)},
    {"f32 action_stride % 4 == 2", cartpole(), stride(ring(), 1026), planned(1)},
    {"f32 action_stride 0 (one slice)", cartpole(), stride(ring(), 0), planned(4)},
    {"f32 d_rec_obs 4 bytes off a 16-byte line", cartpole(), obs_at(ring(), 4), planned(1)},
    {"f32 d_rec_obs 8 bytes off", cartpole(), obs_at(ring(), 8), planned(1)},
    {"f32 d_rec_reward 4 bytes off", cartpole(), reward_at(ring(), 4), planned(1)},
    {"f32 d_rec_reward 8 bytes off", cartpole(), reward_at(ring(), 8), planned(1)},
    {"f32 d_rec_actions aligned (a bookkeeping handle records a ring's)", bookkeeping(cartpole()), rec_actions_at(ring(), 0), planned(4)},
    {"f32 d_rec_actions 4 bytes off", bookkeeping(cartpole()), rec_actions_at(ring(), 4), planned(1)},
    {"f32 d_rec_actions 8 bytes off", bookkeeping(cartpole()), rec_actions_at(ring(), 8), planned(1)},
    {"f32 SAMPLE d_rec_actions 8 bytes off", cartpole(), source(rec_actions_at(ring(), 8), GYMNET_ACTIONS_SAMPLE), unread(planned(1))},
    {"f32 d_rec_done 1 byte off", cartpole(), done_at(ring(), 1), planned(1)},
    {"f32 d_rec_done 2 bytes off", cartpole(), done_at(ring(), 2), planned(1)},
    {"f32 d_rec_done 4 bytes off stays at 4", cartpole(), done_at(ring(), 4), planned(4)},
    {"f32 SAMPLE does not read d_actions: 4 bytes off", cartpole(), source(actions_at(ring(), 4), GYMNET_ACTIONS_SAMPLE), unread(planned(4))},
    {"f32 SAMPLE: null d_actions, odd stride", cartpole(), source(stride(no_actions(ring()), 1025), GYMNET_ACTIONS_SAMPLE), unread(planned(4))},
    {"f32 ACTOR does not read d_actions: 4 bytes off", kDiscrete, actions_at(kActor, 4), unread(planned(4), true)},
    {"f32 EPSILON_GREEDY reads d_actions: 4 bytes off", cartpole(), source(actions_at(ring(), 4), GYMNET_ACTIONS_EPSILON_GREEDY), planned(1)},
    {"f32 lcfg.vec 1 stays 1", cartpole(1024, 1), ring(), planned(1)},
    // ---- Acrobot with lcfg.vec = 2 (streams_fit(2): n % 2, d_actions 8, stride % 2, obs 16, reward 8, done 2, actions 8)
    {"Acrobot every stream aligned", acrobot(), ring(), planned(2)},
    {"Acrobot odd n", acrobot(1023), ring(1023), planned(1)},
    {"Acrobot d_rec_done 1 byte off", acrobot(), done_at(ring(), 1), planned(1)},
    {"Acrobot d_rec_done 2 bytes off stays at 2", acrobot(), done_at(ring(), 2), planned(2)},
    {"Acrobot d_rec_reward 4 bytes off", acrobot(), reward_at(ring(), 4), planned(1)},
    {"Acrobot d_rec_reward 8 bytes off stays at 2", acrobot(), reward_at(ring(), 8), planned(2)},
    {"Acrobot d_actions 8 bytes off stays at 2", acrobot(), actions_at(ring(), 8), planned(2)},
    {"Acrobot d_actions 4 bytes off", acrobot(), actions_at(ring(), 4), planned(1)},
    {"Acrobot d_rec_obs 8 bytes off", acrobot(), obs_at(ring(), 8), planned(1)},
    {"Acrobot odd stride", acrobot(), stride(ring(), 1025), planned(1)},
    // ---- float64 CartPole, lcfg.vec = 2: the fat form (4) where sstride % 4 == 0 and streams_fit(4), else streams_fit(2), else 1
    {"f64 n 8192: lcfg.vec 2 with everything fitting is raised to 4", cartpole64(8192), ring(8192), planned(4)},
    {"f64 n 4102", cartpole64(4102), ring(4102), planned(2)},
    {"f64 n 1021", cartpole64(1021), ring(1021), planned(1)},
    {"f64 sstride % 4 == 2, everything else fitting", [] { FusedFacts f = cartpole64(8192); f.sstride = 8194; return f; }(), ring(8192), planned(2)},
    {"f64 lcfg.vec 1 with everything fitting stays 1", cartpole64(8192, 1), ring(8192), planned(1)},
    {"f64 d_rec_reward 8 bytes off gives 2, not 4", cartpole64(8192), reward_at(ring(8192), 8), planned(2)},
    {"f64 d_rec_reward 4 bytes off", cartpole64(8192), reward_at(ring(8192), 4), planned(1)},
    {"f64 d_rec_done 2 bytes off gives 2", cartpole64(8192), done_at(ring(8192), 2), planned(2)},
    {"f64 d_rec_done 1 byte off", cartpole64(8192), done_at(ring(8192), 1), planned(1)},
    {"f64 d_rec_obs 8 bytes off", cartpole64(8192), obs_at(ring(8192), 8), planned(1)},
    {"f64 d_actions 8 bytes off gives 2", cartpole64(8192), actions_at(ring(8192), 8), planned(2)},
    {"f64 stride % 4 == 2 gives 2", cartpole64(8192), stride(ring(8192), 8194), planned(2)},
    {"f64 SAMPLE: d_actions 4 bytes off does not matter", cartpole64(8192), source(actions_at(ring(8192), 4), GYMNET_ACTIONS_SAMPLE), unread(planned(4))},
    // ---- refusals, each the first failure, in the order the call reports them
    {"spec is null", cartpole(), null_spec(ring()), refused(ARG, "spec is null")},
    {"spec mis-sized", cartpole(), struct_size(ring(), 136), refused(ARG, "spec.struct_size 136 != 144 (ABI mismatch)")},
    {"logp: ring source", kDiscrete, logp_at(ring(), 0), refused(ARG, "d_rec_logp: log-probabilities are recorded where the actor chooses (action_source GYMNET_ACTIONS_ACTOR), not 0")},
    {"logp: no actor", cartpole(), logp_at(kActor, 0), refused(ARG, "no actor configured (gymnet_vecenv_actor_config)")},
    {"logp: no actor, Box env", pendulum(), logp_at(kActor, 0), refused(ARG, "no actor configured (gymnet_vecenv_actor_box_config)")},
    {"logp: Box actor", kBox, logp_at(kActor, 0), refused(ARG, "d_rec_logp: this handle's actor chooses Box actions; a log-probability belongs to a Discrete actor")},
    {"logp: 2 bytes off", kDiscrete, logp_at(kActor, 2), refused(ARG, "d_rec_logp must be 4-byte aligned")},
    {"logp: 4 bytes off a line is served", kDiscrete, logp_at(kActor, 4), unread(planned(4), true)},
    {"value: sampled source", kCritic, value_at(source(ring(), GYMNET_ACTIONS_SAMPLE), 0), refused(ARG, "d_rec_value: values are recorded where the actor chooses (action_source GYMNET_ACTIONS_ACTOR), not 1")},
    {"value: no actor", cartpole(), value_at(kActor, 0), refused(ARG, "no actor configured (gymnet_vecenv_actor_config)")},
    {"value: Box actor", kBox, value_at(kActor, 0), refused(ARG, "d_rec_value: this handle's actor chooses Box actions; the fused rollout records values for a Discrete actor (gymnet_vecenv_actor_value_device serves a Box actor)")},
    {"value: no critic", kDiscrete, value_at(kActor, 0), refused(ARG, "d_rec_value: no critic configured (gymnet_vecenv_actor_critic_config)")},
    {"value: logp 1 byte off", kCritic, value_at(logp_at(kActor, 1), 0), refused(ARG, "d_rec_logp must be 4-byte aligned")},
    {"value: 2 bytes off", kCritic, value_at(logp_at(kActor, 0), 2), refused(ARG, "d_rec_value must be 4-byte aligned")},
    {"value without logp is served", kCritic, value_at(kActor, 4), unread(planned(4), true)},
    {"action_source -1", cartpole(), source(ring(), -1), refused(ARG, "bad action_source -1")},
    {"action_source 4", cartpole(), source(ring(), 4), refused(ARG, "bad action_source 4")},
    {"ring without d_actions", cartpole(), no_actions(ring()), refused(ARG, "d_actions is null")},
    {"epsilon-greedy without d_actions", cartpole(), source(no_actions(ring()), GYMNET_ACTIONS_EPSILON_GREEDY), refused(ARG, "d_actions is null")},
    {"steps -1", cartpole(), steps(ring(), -1), refused(ARG, "bad steps/ring/action_stride")},
    {"ring 0", cartpole(), ring_len(ring(), 0), refused(ARG, "bad steps/ring/action_stride")},
    {"action_stride -1", cartpole(), stride(ring(), -1), refused(ARG, "bad steps/ring/action_stride")},
    {"SAMPLE: ring 0 and stride -1 are not read", cartpole(), source(stride(ring_len(ring(), 0), -1), GYMNET_ACTIONS_SAMPLE), unread(planned(4))},
    {"steps INT32_MAX", cartpole(), steps(ring(), kMax), planned(4, (uint64_t)kMax)},
    {"steps INT32_MAX + 1", cartpole(), steps(ring(), kMax + 1), refused(ARG, "steps must fit an int32 (episode records carry the step index)")},
    {"record_flags 2", cartpole(), flags(ring(), 2), refused(ARG, "unknown record_flags bits 0x2")},
    {"record_flags 3", cartpole(), flags(ring(), 3), refused(ARG, "unknown record_flags bits 0x3")},
    {"record_flags NO_OVERFLOW is served", cartpole(), flags(ring(), GYMNET_RECORDS_NO_OVERFLOW), planned(4)},
    {"epsilon-greedy on a Box space", pendulum(), source(ring(), GYMNET_ACTIONS_EPSILON_GREEDY), refused(UNS, "epsilon-greedy composition is defined for Discrete action spaces")},
    {"epsilon-greedy epsilon 0", cartpole(), epsilon(source(ring(), GYMNET_ACTIONS_EPSILON_GREEDY), 0.0f), planned(4)},
    {"epsilon-greedy epsilon 1", cartpole(), epsilon(source(ring(), GYMNET_ACTIONS_EPSILON_GREEDY), 1.0f), planned(4)},
    {"epsilon-greedy epsilon just below 0", cartpole(), epsilon(source(ring(), GYMNET_ACTIONS_EPSILON_GREEDY), kBelow0), refused(ARG, "epsilon must be in [0, 1]")},
    {"epsilon-greedy epsilon just above 1", cartpole(), epsilon(source(ring(), GYMNET_ACTIONS_EPSILON_GREEDY), kAbove1), refused(ARG, "epsilon must be in [0, 1]")},
    {"epsilon-greedy epsilon NaN", cartpole(), epsilon(source(ring(), GYMNET_ACTIONS_EPSILON_GREEDY), kNaN), refused(ARG, "epsilon must be in [0, 1]")},
    {"ring: epsilon is not read", cartpole(), epsilon(ring(), kNaN), planned(4)},
    {"actor with frame skip", kDiscrete, held(kActor, 1), refused(UNS, "the fused actor rollout has no frame skip: run the unfused loop, one decision at a time (actor_act_device, step_repeat_device, actor_push_device)")},
    // (INT32_MAX is prime: no held > 0 reaches steps * (held + 1) == INT32_MAX; these are the nearest products on either side)
    {"steps * (held + 1) == INT32_MAX - 1", cartpole(), held(steps(ring(), 1073741823), 1), planned(4, 2147483646u, 1073741823u)},
    {"steps * (held + 1) == INT32_MAX + 1", cartpole(), held(steps(ring(), 1073741824), 1), refused(ARG, "steps * (repeat + 1) must fit an int32")},
    {"steps * (held + 1) == INT32_MAX + 2, held 2", cartpole(), held(steps(ring(), 715827883), 2), refused(ARG, "steps * (repeat + 1) must fit an int32")},
    {"held 255: 8 decisions are 2048 ticks", cartpole(), held(ring(), 255), planned(4, 2048, 2040)},
    {"actor on a float64 handle", with_actor(cartpole64(8192), ActorKind::Discrete), source(ring(8192), GYMNET_ACTIONS_ACTOR), refused(UNS, "the fused actor rollout runs float32 handles (float64: act / step / push)")},
    {"actor epsilon 0", kDiscrete, epsilon(kActor, 0.0f), unread(planned(4), true)},
    {"actor epsilon 1", kDiscrete, epsilon(kActor, 1.0f), unread(planned(4), true)},
    {"actor epsilon just below 0", kDiscrete, epsilon(kActor, kBelow0), refused(ARG, "epsilon must be in [0, 1]")},
    {"actor epsilon just above 1", kDiscrete, epsilon(kActor, kAbove1), refused(ARG, "epsilon must be in [0, 1]")},
    {"actor epsilon NaN", kDiscrete, epsilon(kActor, kNaN), refused(ARG, "epsilon must be in [0, 1]")},
    {"actor source without an actor", cartpole(), kActor, refused(ARG, "no actor configured (gymnet_vecenv_actor_config)")},
    {"actor source without an actor, Box env", pendulum(), kActor, refused(ARG, "no actor configured (gymnet_vecenv_actor_box_config)")},
    {"stale actor", with_actor(cartpole(), ActorKind::Discrete, false), kActor, refused(ARG, "the actor's history is stale: reset the actor (or push) before an actor rollout")},
    {"stale Box actor", with_actor(pendulum(), ActorKind::Box, false), kActor, refused(ARG, "the actor's history is stale: reset the actor (or push) before an actor rollout")},
    {"Box actor is served", kBox, kActor, unread(planned(4), true)},
    {"VALIDATE_ACTIONS with a ring", validating(cartpole()), ring(), refused(UNS, "VALIDATE_ACTIONS is per step; use gymnet_vecenv_rollout_device (sampled actions are valid by construction)")},
    {"VALIDATE_ACTIONS with epsilon-greedy", validating(cartpole()), source(ring(), GYMNET_ACTIONS_EPSILON_GREEDY), refused(UNS, "VALIDATE_ACTIONS is per step; use gymnet_vecenv_rollout_device (sampled actions are valid by construction)")},
    {"VALIDATE_ACTIONS, the slice validated by the caller", validating(cartpole()), held(steps(ring(), 1), 3, true), planned(4, 4, 3)},
    {"VALIDATE_ACTIONS with sampled actions", validating(cartpole()), source(ring(), GYMNET_ACTIONS_SAMPLE), unread(planned(4))},
    {"VALIDATE_ACTIONS with the actor", validating(kDiscrete), kActor, unread(planned(4), true)},
    {"episodes on a lean handle", cartpole(), episodes(ring(), 64), refused(UNS, "episode records need a bookkeeping handle (GYMNET_FLAG_EPISODE_STATS / DONE_LIST / FINAL_OBS)")},
    {"episode returns without statistics", bookkeeping(cartpole(), false), episodes(ring(), 64), refused(UNS, "episode return / length records need GYMNET_FLAG_EPISODE_STATS")},
    {"ep_capacity -1", bookkeeping(cartpole()), episodes(ring(), -1), refused(ARG, "episode records need ep_capacity >= 0 and d_ep_count")},
    {"episodes without d_ep_count", bookkeeping(cartpole()), episodes(ring(), 64, true, false), refused(ARG, "episode records need ep_capacity >= 0 and d_ep_count")},
    {"d_rec_actions of a lean ring rollout", cartpole(), rec_actions_at(ring(), 0), refused(UNS, "d_rec_actions: the actions of a plain ring rollout ARE the ring (recorded for sampled / epsilon-greedy actions and on bookkeeping handles)")},
    {"d_rec_actions of a lean sampled rollout is served", cartpole(), source(rec_actions_at(ring(), 0), GYMNET_ACTIONS_SAMPLE), unread(planned(4))},
    {"d_rec_actions of a lean epsilon-greedy rollout is served", cartpole(), source(rec_actions_at(ring(), 0), GYMNET_ACTIONS_EPSILON_GREEDY), planned(4)},
    // ---- steps == 0: nothing launched, no tick
    {"steps 0", cartpole(), steps(ring(), 0), nothing_to_do(false)},
    {"steps 0 with episode pointers", bookkeeping(cartpole()), episodes(steps(ring(), 0), 64), nothing_to_do(true)},
    {"steps 0 with a logp pointer", kDiscrete, logp_at(steps(kActor, 0), 0), [] { Want w = nothing_to_do(false, false); w.plan.actor = true; return w; }()},
    {"steps 0 with frame skip", cartpole(), held(steps(ring(), 0), 7), nothing_to_do(false)},
    // ---- doubly wrong calls: the first refusal in the order above is the one reported
    {"bad action_source and null d_actions", cartpole(), source(no_actions(ring()), 7), refused(ARG, "bad action_source 7")},
    {"rec_value on a Box actor with a misaligned rec_logp", kBox, value_at(logp_at(kActor, 2), 0), refused(ARG, "d_rec_value: this handle's actor chooses Box actions; the fused rollout records values for a Discrete actor (gymnet_vecenv_actor_value_device serves a Box actor)")},
    {"stale actor with VALIDATE_ACTIONS", validating(with_actor(cartpole(), ActorKind::Discrete, false)), kActor, refused(ARG, "the actor's history is stale: reset the actor (or push) before an actor rollout")},
    {"frame skip with the actor on a float64 handle", with_actor(cartpole64(8192), ActorKind::Discrete), held(source(ring(8192), GYMNET_ACTIONS_ACTOR), 2), refused(UNS, "the fused actor rollout has no frame skip: run the unfused loop, one decision at a time (actor_act_device, step_repeat_device, actor_push_device)")},
    {"null spec with a record pointer", kDiscrete, null_spec(logp_at(kActor, 2)), refused(ARG, "spec is null")},
    {"mis-sized spec with a value pointer", cartpole(), struct_size(value_at(ring(), 1), 8), refused(ARG, "spec.struct_size 8 != 144 (ABI mismatch)")},
    {"logp pointer with action_source 7", kDiscrete, logp_at(source(ring(), 7), 0), refused(ARG, "d_rec_logp: log-probabilities are recorded where the actor chooses (action_source GYMNET_ACTIONS_ACTOR), not 7")},
    {"logp pointer misaligned and the actor stale", with_actor(cartpole(), ActorKind::Discrete, false), logp_at(kActor, 2), refused(ARG, "d_rec_logp must be 4-byte aligned")},
    {"value: no critic and the value pointer misaligned", kDiscrete, value_at(kActor, 2), refused(ARG, "d_rec_value: no critic configured (gymnet_vecenv_actor_critic_config)")},
    {"value: no critic and the logp pointer misaligned", kDiscrete, value_at(logp_at(kActor, 1), 0), refused(ARG, "d_rec_value: no critic configured (gymnet_vecenv_actor_critic_config)")},
    {"actor with frame skip and a product beyond int32", kDiscrete, held(steps(kActor, 1073741824), 1), refused(UNS, "the fused actor rollout has no frame skip: run the unfused loop, one decision at a time (actor_act_device, step_repeat_device, actor_push_device)")},
    {"null d_actions and steps -1", cartpole(), steps(no_actions(ring()), -1), refused(ARG, "d_actions is null")},
    {"steps -1 and record_flags 2", cartpole(), flags(steps(ring(), -1), 2), refused(ARG, "bad steps/ring/action_stride")},
    {"steps beyond int32 and record_flags 2", cartpole(), flags(steps(ring(), kMax + 1), 2), refused(ARG, "steps must fit an int32 (episode records carry the step index)")},
    {"record_flags 2 and epsilon-greedy on a Box space", pendulum(), flags(source(ring(), GYMNET_ACTIONS_EPSILON_GREEDY), 2), refused(ARG, "unknown record_flags bits 0x2")},
    {"epsilon-greedy on a Box space without d_actions", pendulum(), source(no_actions(ring()), GYMNET_ACTIONS_EPSILON_GREEDY), refused(ARG, "d_actions is null")},
    {"epsilon-greedy on a Box space with epsilon 2", pendulum(), epsilon(source(ring(), GYMNET_ACTIONS_EPSILON_GREEDY), 2.0f), refused(UNS, "epsilon-greedy composition is defined for Discrete action spaces")},
    {"actor: float64 and epsilon 2", with_actor(cartpole64(8192), ActorKind::Discrete), epsilon(source(ring(8192), GYMNET_ACTIONS_ACTOR), 2.0f), refused(UNS, "the fused actor rollout runs float32 handles (float64: act / step / push)")},
    {"actor: epsilon 2 and no actor", cartpole(), epsilon(kActor, 2.0f), refused(ARG, "epsilon must be in [0, 1]")},
    {"VALIDATE_ACTIONS and episodes on a lean handle", validating(cartpole()), episodes(ring(), 64), refused(UNS, "VALIDATE_ACTIONS is per step; use gymnet_vecenv_rollout_device (sampled actions are valid by construction)")},
    {"episodes and d_rec_actions on a lean handle", cartpole(), episodes(rec_actions_at(ring(), 0), 64), refused(UNS, "episode records need a bookkeeping handle (GYMNET_FLAG_EPISODE_STATS / DONE_LIST / FINAL_OBS)")},
    {"no statistics and ep_capacity -1", bookkeeping(cartpole(), false), episodes(ring(), -1), refused(UNS, "episode return / length records need GYMNET_FLAG_EPISODE_STATS")},
    {"steps 0 and episodes on a lean handle", cartpole(), episodes(steps(ring(), 0), 64), refused(UNS, "episode records need a bookkeeping handle (GYMNET_FLAG_EPISODE_STATS / DONE_LIST / FINAL_OBS)")},
    {"held overflow and the steps themselves beyond int32", cartpole(), held(steps(ring(), kMax + 1), 1), refused(ARG, "steps must fit an int32 (episode records carry the step index)")},
    // ---- the segment block: cap = 2 * ceil(capacity / 256) + 64, one overflow segment of `capacity`; grown where the handle's is smaller
    {"capacity 0", bookkeeping(cartpole()), episodes(ring(), 0), with_segments(planned(4), 64, 0, true, 0)},
    {"capacity 1", bookkeeping(cartpole()), episodes(ring(), 1), with_segments(planned(4), 66, 1, true, 1)},
    {"capacity kShards", bookkeeping(cartpole()), episodes(ring(), 256), with_segments(planned(4), 66, 256, true, 256)},
    {"capacity kShards + 1", bookkeeping(cartpole()), episodes(ring(), 257), with_segments(planned(4), 68, 257, true, 257)},
    {"step and lane records without statistics", bookkeeping(cartpole(), false), episodes(ring(), 64, false), with_segments(planned(4), 66, 64, true, 64)},
    {"held block fits exactly", holding(bookkeeping(cartpole()), 66, 256), episodes(ring(), 256), with_segments(planned(4), 66, 256, false, 256)},
    {"held block one record short in the overflow segment", holding(bookkeeping(cartpole()), 68, 256), episodes(ring(), 257), with_segments(planned(4), 68, 257, true, 257)},
    {"held block one record short per shard", holding(bookkeeping(cartpole()), 66, 300), episodes(ring(), 257), with_segments(planned(4), 68, 257, true, 257)},
    {"held block larger: kept, ov_cap = min(ep_capacity, held)", holding(bookkeeping(cartpole()), 68, 300), episodes(ring(), 100), with_segments(planned(4), 68, 300, false, 100)},
    {"held shards large, overflow segment small", holding(bookkeeping(cartpole()), 200, 10), episodes(ring(), 100), with_segments(planned(4), 66, 100, true, 100)},
    {"capacities without a block count for nothing", [] { FusedFacts f = holding(bookkeeping(cartpole()), 68, 300); f.has_segments = false; return f; }(), episodes(ring(), 100), with_segments(planned(4), 66, 100, true, 100)},
    {"episodes with frame skip", bookkeeping(cartpole()), held(episodes(ring(), 256), 3), with_segments(planned(4, 32, 24), 66, 256, true, 256)},
};

bool same_plan(const FusedPlan &a, const FusedPlan &b) {
    return a.ring_read == b.ring_read && a.actor == b.actor && a.episodes == b.episodes && a.zero_steps == b.zero_steps && a.vec == b.vec &&
           a.segments.cap == b.segments.cap && a.segments.ov_cap == b.segments.ov_cap && a.grow == b.grow && a.ov_cap == b.ov_cap &&
           a.ticks == b.ticks && a.held_ticks == b.held_ticks;
}

void print_plan(const char *tag, const FusedPlan &p) {
    std::printf("    %s ring_read %d actor %d episodes %d zero_steps %d vec %d segments (%lld, %lld) grow %d ov_cap %lld ticks %llu held_ticks %llu\n", tag,
                p.ring_read, p.actor, p.episodes, p.zero_steps, p.vec, (long long)p.segments.cap, (long long)p.segments.ov_cap, p.grow, (long long)p.ov_cap,
                (unsigned long long)p.ticks, (unsigned long long)p.held_ticks);
}

}  // namespace

int main() {
    int rows = 0, failed = 0;
    for (const Row &row : kRows) {
        FusedRequest rq;
        rq.spec = row.a.null_spec ? nullptr : &row.a.sp;
        rq.held = row.a.held; rq.validated = row.a.validated;
        rq.rec_logp = static_cast<float *>(row.a.rec_logp); rq.rec_value = static_cast<float *>(row.a.rec_value);
        const FusedOutcome got = plan_fused_rollout(row.f, rq);
        ++rows;
        bool ok = got.status == row.w.status;
        if (ok && got.status != GYMNET_OK) ok = std::strcmp(got.text, row.w.text) == 0;
        if (ok && got.status == GYMNET_OK) ok = same_plan(got.plan, row.w.plan);
        if (!ok) {
            ++failed;
            std::printf("FAILED %s: status %d (want %d)\n    got  \"%s\"\n    want \"%s\"\n", row.name, got.status, row.w.status, got.text, row.w.text);
            if (got.status == GYMNET_OK) print_plan("got ", got.plan);
            if (row.w.status == GYMNET_OK) print_plan("want", row.w.plan);
        }
    }
    // EpisodeSegments against the two formulas it replaced: ensure_episode_segments' byte count
    //   (kShards * cap + capacity) * 16 + (kShards + 1) * kCountStride * 4 + 8
    // and rollout_fused_typed's carving: one = (kShards * cap + ov) * 4; t at 0, lane at one, return at 2 one, length at 3 one, counters at 4 one
    struct Seg { int64_t cap, ov; size_t one, bytes; };
    for (const Seg &s : {Seg{66, 256, 68608, 290888}, Seg{68, 257, 70660, 299096}}) {
        const EpisodeSegments e{s.cap, s.ov};
        ++rows;
        const bool ok = e.bytes() == s.bytes && e.offset(0) == 0 && e.offset(1) == s.one && e.offset(2) == 2 * s.one && e.offset(3) == 3 * s.one &&
                        e.counters_offset() == 4 * s.one && e.counters_offset() + (size_t)(kShards + 1) * kCountStride * 4 + 8 == e.bytes();
        if (!ok) { ++failed; std::printf("FAILED segments (%lld, %lld): bytes %zu one %zu\n", (long long)s.cap, (long long)s.ov, e.bytes(), e.offset(1)); }
    }
    std::printf("%d rows, %d failed\n", rows, failed);
    return failed ? 1 : 0;
}
