// rollout_plan_logd_test.cpp — the Box actor's log-density request in the fused rollout's plan (gym.net_amd/csrc/rollout_plan.hpp
// box_record_pointers), held to a table on the CPU as tests/cpp/rollout_plan_test.cpp holds the rest: every new refusal as the first
// failure, each pair of neighbours in the documented order, d_rec_value alone through the new request, and a sample of the old table's
// rows planned with the new fields at their defaults.  g++ -std=c++17, no library, no HIP.  Pointers are integers here.
//
// Expected values are the contract of gymnet_vecenv_rollout_fused_box_logd_device in include/gymnet_amd.h (the order: action source, no
// actor, Discrete actor, sigma, critic, d_rec_logd's alignment, d_rec_value's) and, for the old rows, the strings of
// tests/cpp/rollout_plan_test.cpp — never the code under test.
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

void *at(int stream, int64_t off) { return reinterpret_cast<void *>((uintptr_t)0x7f0000000000ull + (uintptr_t)stream * 0x100000u + (uintptr_t)off); }
enum { ACT = 1, OBS, REW, DONE, RACT, LOGP, VALUE, LOGD };

FusedFacts handle(bool box, int64_t n = 1024) {
    FusedFacts f;
    f.n = n; f.sstride = (n + 63) / 64 * 64; f.alias = !box; f.vec = 4; f.box_action = box;
    return f;
}
FusedFacts with_actor(FusedFacts f, ActorKind kind, float sigma, bool critic = false, bool current = true) {
    f.actor.kind = kind; f.actor.critic = critic; f.actor.current = current; f.actor.box_sigma = sigma;
    return f;
}

struct Ask {
    gymnet_rollout_spec sp{};
    bool null_spec = false;
    int32_t held = 0;
    void *rec_logp = nullptr, *rec_value = nullptr, *rec_logd = nullptr;
    bool box_value = false;
};
Ask actor_rollout(int32_t source = GYMNET_ACTIONS_ACTOR) {
    Ask a;
    a.sp.struct_size = sizeof a.sp; a.sp.action_source = source;
    a.sp.d_actions = at(ACT, 0); a.sp.steps = 8; a.sp.action_stride = 1024; a.sp.ring = 1;
    a.sp.d_rec_obs = at(OBS, 0); a.sp.d_rec_reward = static_cast<float *>(at(REW, 0)); a.sp.d_rec_done = static_cast<uint8_t *>(at(DONE, 0));
    return a;
}
Ask logd_at(Ask a, int64_t off) { a.rec_logd = at(LOGD, off); return a; }
// d_rec_value as gymnet_vecenv_rollout_fused_box_logd_device hands it down ...
Ask box_value_at(Ask a, int64_t off) { a.rec_value = at(VALUE, off); a.box_value = true; return a; }
// ... and as gymnet_vecenv_rollout_fused_value_device does
Ask old_value_at(Ask a, int64_t off) { a.rec_value = at(VALUE, off); return a; }
Ask logp_at(Ask a, int64_t off) { a.rec_logp = at(LOGP, off); return a; }
Ask held(Ask a, int32_t hd) { a.held = hd; return a; }
Ask steps(Ask a, int64_t s) { a.sp.steps = s; return a; }
Ask epsilon(Ask a, float e) { a.sp.epsilon = e; return a; }
Ask null_spec(Ask a) { a.null_spec = true; return a; }

struct Want { int status = GYMNET_OK; std::string text; bool zero_steps = false; };
Want refused(const char *text, int status = GYMNET_ERR_INVALID_ARG) { return Want{status, text, false}; }
Want served() { return Want{}; }

struct Row { const char *name; FusedFacts f; Ask a; Want w; };

const float kTiny = std::numeric_limits<float>::denorm_min();          // 1.0f / kTiny overflows
const float kTooSmall = std::ldexp(1.0f, -128);                        // 1 / sigma = 2^128: above FLT_MAX
const float kSmallestOk = std::ldexp(2097153.0f, -149);                // the next float32 (a subnormal): 1 / sigma rounds to a finite value
const FusedFacts kBox = with_actor(handle(true), ActorKind::Box, 0.5f), kBoxCritic = with_actor(handle(true), ActorKind::Box, 0.5f, true);
const FusedFacts kBoxFresh = with_actor(handle(true), ActorKind::Box, 0.0f, true), kBoxTiny = with_actor(handle(true), ActorKind::Box, kTiny, true);
const FusedFacts kDiscrete = with_actor(handle(false), ActorKind::Discrete, 0.0f, true);

#define SRC_LOGD "d_rec_logd: log-densities and values are recorded where the actor chooses (action_source GYMNET_ACTIONS_ACTOR), not "
#define SRC_VALUE "d_rec_value: log-densities and values are recorded where the actor chooses (action_source GYMNET_ACTIONS_ACTOR), not "
#define DISCRETE(what) what ": this handle's actor chooses Discrete actions; a log-density belongs to a Box actor (gymnet_vecenv_rollout_fused_value_device records a Discrete actor's log-probability and value)"
#define SIGMA(what, s) what ": the log-density needs a policy with sigma > 0 and a finite 1 / sigma (gymnet_vecenv_actor_box_set_policy), not " s
#define NO_CRITIC "d_rec_value: no critic configured (gymnet_vecenv_actor_critic_config)"
#define STALE "the actor's history is stale: reset the actor (or push) before an actor rollout"

const std::vector<Row> kRows = {
    // ---- each refusal as the first failure
    {"logd: ring source", kBox, logd_at(actor_rollout(GYMNET_ACTIONS_RING), 0), refused(SRC_LOGD "0")},
    {"logd: sampled source", kBox, logd_at(actor_rollout(GYMNET_ACTIONS_SAMPLE), 0), refused(SRC_LOGD "1")},
    {"value alone: epsilon-greedy source", kBoxCritic, box_value_at(actor_rollout(GYMNET_ACTIONS_EPSILON_GREEDY), 0), refused(SRC_VALUE "2")},
    {"logd: no actor, Box env", handle(true), logd_at(actor_rollout(), 0), refused("no actor configured (gymnet_vecenv_actor_box_config)")},
    {"logd: no actor, Discrete env", handle(false), logd_at(actor_rollout(), 0), refused("no actor configured (gymnet_vecenv_actor_config)")},
    {"logd: Discrete actor", kDiscrete, logd_at(actor_rollout(), 0), refused(DISCRETE("d_rec_logd"))},
    {"value alone: Discrete actor", kDiscrete, box_value_at(actor_rollout(), 0), refused(DISCRETE("d_rec_value"))},
    {"logd: sigma 0, the fresh default", kBoxFresh, logd_at(actor_rollout(), 0), refused(SIGMA("d_rec_logd", "0"))},
    {"logd: 1 / sigma overflows", kBoxTiny, logd_at(actor_rollout(), 0), refused(SIGMA("d_rec_logd", "1.4013e-45"))},
    {"value alone: sigma 0", kBoxFresh, box_value_at(actor_rollout(), 0), refused(SIGMA("d_rec_value", "0"))},
    {"logd: the smallest sigma with a finite reciprocal is served", with_actor(handle(true), ActorKind::Box, kSmallestOk), logd_at(actor_rollout(), 0), served()},
    {"logd: a large sigma is served", with_actor(handle(true), ActorKind::Box, 3.0e38f), logd_at(actor_rollout(), 0), served()},
    {"value: no critic", kBox, box_value_at(logd_at(actor_rollout(), 0), 0), refused(NO_CRITIC)},
    {"value alone: no critic", kBox, box_value_at(actor_rollout(), 0), refused(NO_CRITIC)},
    {"logd: 2 bytes off", kBox, logd_at(actor_rollout(), 2), refused("d_rec_logd must be 4-byte aligned")},
    {"logd: 1 byte off", kBox, logd_at(actor_rollout(), 1), refused("d_rec_logd must be 4-byte aligned")},
    {"value: 2 bytes off", kBoxCritic, box_value_at(logd_at(actor_rollout(), 0), 2), refused("d_rec_value must be 4-byte aligned")},
    {"value alone: 3 bytes off", kBoxCritic, box_value_at(actor_rollout(), 3), refused("d_rec_value must be 4-byte aligned")},
    // ---- served
    {"logd alone, 4 bytes off a line", kBox, logd_at(actor_rollout(), 4), served()},
    {"logd alone needs no critic", kBox, logd_at(actor_rollout(), 0), served()},
    {"logd and value", kBoxCritic, box_value_at(logd_at(actor_rollout(), 0), 4), served()},
    {"value alone through the new request", kBoxCritic, box_value_at(actor_rollout(), 0), served()},
    {"steps 0 with a logd pointer", kBox, logd_at(steps(actor_rollout(), 0), 0), Want{GYMNET_OK, "", true}},
    // ---- the order: each pair of neighbours wrong at once reports the earlier one
    {"null spec comes first", kBox, null_spec(logd_at(actor_rollout(), 2)), refused("spec is null")},
    {"source before no actor", handle(true), logd_at(actor_rollout(GYMNET_ACTIONS_RING), 0), refused(SRC_LOGD "0")},
    {"source 7 is the new check's, not the rollout's", kBox, logd_at(actor_rollout(7), 0), refused(SRC_LOGD "7")},
    {"no actor before sigma (a handle without an actor has sigma 0)", handle(true), box_value_at(logd_at(actor_rollout(), 2), 2), refused("no actor configured (gymnet_vecenv_actor_box_config)")},
    {"Discrete before sigma", kDiscrete, logd_at(actor_rollout(), 2), refused(DISCRETE("d_rec_logd"))},
    {"sigma before critic", with_actor(handle(true), ActorKind::Box, 0.0f), box_value_at(logd_at(actor_rollout(), 0), 0), refused(SIGMA("d_rec_logd", "0"))},
    {"critic before logd's alignment", kBox, box_value_at(logd_at(actor_rollout(), 2), 0), refused(NO_CRITIC)},
    {"logd's alignment before value's", kBoxCritic, box_value_at(logd_at(actor_rollout(), 2), 2), refused("d_rec_logd must be 4-byte aligned")},
    {"value's alignment before the rollout's own checks", with_actor(handle(true), ActorKind::Box, 0.5f, true, false), box_value_at(logd_at(actor_rollout(), 0), 2), refused("d_rec_value must be 4-byte aligned")},
    // ---- then the rollout's own checks apply
    {"stale history", with_actor(handle(true), ActorKind::Box, 0.5f, true, false), box_value_at(logd_at(actor_rollout(), 0), 0), refused(STALE)},
    {"frame skip", kBox, held(logd_at(actor_rollout(), 0), 1), refused("the fused actor rollout has no frame skip: run the unfused loop, one decision at a time (actor_act_device, step_repeat_device, actor_push_device)", GYMNET_ERR_UNSUPPORTED)},
    {"epsilon 2", kBox, epsilon(logd_at(actor_rollout(), 0), 2.0f), refused("epsilon must be in [0, 1]")},
    {"a float64 handle", [] { FusedFacts f = with_actor(handle(true), ActorKind::Box, 0.5f); f.f64 = true; return f; }(), logd_at(actor_rollout(), 0), refused("the fused actor rollout runs float32 handles (float64: act / step / push)", GYMNET_ERR_UNSUPPORTED)},
    // ---- the old calls keep refusing a Box actor: rec_value without box_value is gymnet_vecenv_rollout_fused_value_device's
    {"old value call on a Box actor with a critic and sigma", kBoxCritic, old_value_at(actor_rollout(), 0), refused("d_rec_value: this handle's actor chooses Box actions; the fused rollout records values for a Discrete actor (gymnet_vecenv_actor_value_device serves a Box actor)")},
    {"old logp call on a Box actor", kBoxCritic, logp_at(actor_rollout(), 0), refused("d_rec_logp: this handle's actor chooses Box actions; a log-probability belongs to a Discrete actor")},
    {"old value call with a misaligned logp on a Box actor", kBoxCritic, old_value_at(logp_at(actor_rollout(), 2), 0), refused("d_rec_value: this handle's actor chooses Box actions; the fused rollout records values for a Discrete actor (gymnet_vecenv_actor_value_device serves a Box actor)")},
    {"old value call on a Discrete actor is served", kDiscrete, old_value_at(actor_rollout(), 4), served()},
    {"old logp call on a Discrete actor, 2 bytes off", kDiscrete, logp_at(actor_rollout(), 2), refused("d_rec_logp must be 4-byte aligned")},
    {"plain actor rollout of a Box actor with sigma 0", kBoxFresh, actor_rollout(), served()},
    {"plain ring rollout", handle(false), actor_rollout(GYMNET_ACTIONS_RING), served()},
};

bool same_plan(const FusedPlan &a, const FusedPlan &b) {
    return a.ring_read == b.ring_read && a.actor == b.actor && a.episodes == b.episodes && a.zero_steps == b.zero_steps && a.vec == b.vec &&
           a.segments.cap == b.segments.cap && a.segments.ov_cap == b.segments.ov_cap && a.grow == b.grow && a.ov_cap == b.ov_cap &&
           a.ticks == b.ticks && a.held_ticks == b.held_ticks;
}

FusedRequest request(const Ask &a) {
    FusedRequest rq;
    rq.spec = a.null_spec ? nullptr : &a.sp;
    rq.held = a.held;
    rq.rec_logp = static_cast<float *>(a.rec_logp); rq.rec_value = static_cast<float *>(a.rec_value);
    rq.rec_logd = static_cast<float *>(a.rec_logd); rq.box_value = a.box_value;
    return rq;
}

}  // namespace

int main() {
    int rows = 0, failed = 0;
    for (const Row &row : kRows) {
        const FusedOutcome got = plan_fused_rollout(row.f, request(row.a));
        ++rows;
        bool ok = got.status == row.w.status;
        if (ok && got.status != GYMNET_OK) ok = row.w.text == got.text;
        if (ok && got.status == GYMNET_OK) ok = got.plan.zero_steps == row.w.zero_steps && got.plan.actor == (row.a.sp.action_source == GYMNET_ACTIONS_ACTOR);
        if (!ok) {
            ++failed;
            std::printf("FAILED %s: status %d (want %d)\n    got  \"%s\"\n    want \"%s\"\n", row.name, got.status, row.w.status, got.text, row.w.text.c_str());
        }
    }
    // a served logd request plans what the plain actor rollout of the same handle plans: the record pointers change no field of the plan
    for (const Ask &a : {logd_at(actor_rollout(), 0), box_value_at(logd_at(actor_rollout(), 0), 0), box_value_at(actor_rollout(), 0)}) {
        const FusedOutcome with = plan_fused_rollout(kBoxCritic, request(a)), plain = plan_fused_rollout(kBoxCritic, request(actor_rollout()));
        ++rows;
        if (!(with.status == GYMNET_OK && plain.status == GYMNET_OK && same_plan(with.plan, plain.plan) && with.plan.actor && with.plan.ticks == 8)) {
            ++failed;
            std::printf("FAILED a served request's plan differs from the plain rollout's\n");
        }
    }
    // the new fields at their defaults: the sigma a handle happens to carry changes nothing for the old requests
    for (const float sigma : {0.0f, 0.5f, kTiny}) {
        for (const Ask &a : {actor_rollout(), old_value_at(actor_rollout(), 0), logp_at(actor_rollout(), 2), held(actor_rollout(), 1), actor_rollout(GYMNET_ACTIONS_SAMPLE)}) {
            for (const ActorKind kind : {ActorKind::Box, ActorKind::Discrete}) {
                const FusedFacts zero = with_actor(handle(kind == ActorKind::Box), kind, 0.0f, true), f = with_actor(handle(kind == ActorKind::Box), kind, sigma, true);
                const FusedOutcome want = plan_fused_rollout(zero, request(a)), got = plan_fused_rollout(f, request(a));
                ++rows;
                if (!(want.status == got.status && std::strcmp(want.text, got.text) == 0 && same_plan(want.plan, got.plan))) {
                    ++failed;
                    std::printf("FAILED sigma %g changes an old request: \"%s\" against \"%s\"\n", (double)sigma, got.text, want.text);
                }
            }
        }
    }
    // box_sigma_ok and box_logd_args: the constants in float64, rounded once
    struct S { float sigma; bool ok; };
    for (const S &s : {S{0.0f, false}, S{-0.0f, false}, S{-1.0f, false}, S{kTiny, false}, S{kTooSmall, false}, S{kSmallestOk, true}, S{0.25f, true}, S{1.7f, true},
                       S{std::numeric_limits<float>::max(), true}, S{std::numeric_limits<float>::quiet_NaN(), false}}) {
        ++rows;
        if (box_sigma_ok(s.sigma) != s.ok) { ++failed; std::printf("FAILED box_sigma_ok(%g)\n", (double)s.sigma); }
    }
    for (const float sigma : {0.25f, 0.5f, 0.3f, 1.7f}) {
        const BoxLogd ld = box_logd_args(sigma);
        ++rows;
        if (!(ld.inv_sigma == (float)(1.0 / (double)sigma) && ld.c == (float)(-std::log((double)sigma) - 0.91893853320467274178))) {
            ++failed;
            std::printf("FAILED box_logd_args(%g)\n", (double)sigma);
        }
    }
    {
        const BoxLogd ld = box_logd_args(0.5f);       // 1 / 0.5 and -ln 0.5 - ln(2 pi) / 2 = -0.2257913526...
        ++rows;
        if (!(ld.inv_sigma == 2.0f && ld.c == -0.2257913526447274f)) { ++failed; std::printf("FAILED box_logd_args(0.5): %.9g %.9g\n", (double)ld.inv_sigma, (double)ld.c); }
    }
    std::printf("%d rows, %d failed\n", rows, failed);
    return failed ? 1 : 0;
}
