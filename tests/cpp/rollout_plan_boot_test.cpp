// rollout_plan_boot_test.cpp — the boot request (V(terminal observation) on time-limit rows) in the fused rollout's plan
// (gym.net_amd/csrc/rollout_plan.hpp record_pointers / box_record_pointers / boot_pointer), held to a table on the CPU as
// tests/cpp/rollout_plan_test.cpp holds the rest: every new refusal as the first failure for a Discrete and for a Box actor, each pair of
// neighbours in the documented order, and old requests planned as before with the new fields at their defaults.  g++ -std=c++17, no
// library, no HIP.  Pointers are integers here.
//
// Expected values are the contract of gymnet_vecenv_rollout_fused_value_boot_device / _box_boot_device in include/gymnet_amd.h (the order:
// d_rec_boot without d_rec_value; every check of the forwarding target in its order; no time limit; d_rec_boot's alignment; the rollout's
// own checks) and, for the old rows, the strings of tests/cpp/rollout_plan_test.cpp and rollout_plan_logd_test.cpp — never the code under
// test.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../gym.net_amd/csrc/rollout_plan.hpp"

using namespace gymnet;

namespace {

void *at(int stream, int64_t off) { return reinterpret_cast<void *>((uintptr_t)0x7f0000000000ull + (uintptr_t)stream * 0x100000u + (uintptr_t)off); }
enum { ACT = 1, OBS, REW, DONE, RACT, LOGP, VALUE, LOGD, BOOT };

FusedFacts handle(bool box, int32_t limit, int64_t n = 1024) {
    FusedFacts f;
    f.n = n; f.sstride = (n + 63) / 64 * 64; f.alias = !box; f.vec = 4; f.box_action = box;
    f.extras = limit > 0; f.ep_stats = limit > 0; f.max_episode_steps = limit;
    return f;
}
FusedFacts with_actor(FusedFacts f, ActorKind kind, float sigma, bool critic = true, bool current = true) {
    f.actor.kind = kind; f.actor.critic = critic; f.actor.current = current; f.actor.box_sigma = sigma;
    return f;
}

struct Ask {
    gymnet_rollout_spec sp{};
    bool null_spec = false;
    int32_t held = 0;
    void *rec_logp = nullptr, *rec_value = nullptr, *rec_logd = nullptr, *rec_boot = nullptr;
    bool box_value = false;
};
Ask actor_rollout(int32_t source = GYMNET_ACTIONS_ACTOR) {
    Ask a;
    a.sp.struct_size = sizeof a.sp; a.sp.action_source = source;
    a.sp.d_actions = at(ACT, 0); a.sp.steps = 8; a.sp.action_stride = 1024; a.sp.ring = 1;
    a.sp.d_rec_obs = at(OBS, 0); a.sp.d_rec_reward = static_cast<float *>(at(REW, 0)); a.sp.d_rec_done = static_cast<uint8_t *>(at(DONE, 0));
    return a;
}
Ask logp_at(Ask a, int64_t off) { a.rec_logp = at(LOGP, off); return a; }
Ask logd_at(Ask a, int64_t off) { a.rec_logd = at(LOGD, off); return a; }
Ask value_at(Ask a, int64_t off) { a.rec_value = at(VALUE, off); return a; }
// d_rec_boot as gymnet_vecenv_rollout_fused_value_boot_device hands it down ...
Ask boot_at(Ask a, int64_t off) { a.rec_boot = at(BOOT, off); return a; }
// ... and as gymnet_vecenv_rollout_fused_box_boot_device does: the request is the Box call's whether or not d_rec_value came with it
Ask box_boot_at(Ask a, int64_t off) { a.rec_boot = at(BOOT, off); a.box_value = true; return a; }
Ask box_value_at(Ask a, int64_t off) { a.rec_value = at(VALUE, off); a.box_value = true; return a; }
Ask held(Ask a, int32_t hd) { a.held = hd; return a; }
Ask steps(Ask a, int64_t s) { a.sp.steps = s; return a; }
Ask null_spec(Ask a) { a.null_spec = true; return a; }

struct Want { int status = GYMNET_OK; std::string text; bool zero_steps = false; };
Want refused(const char *text, int status = GYMNET_ERR_INVALID_ARG) { return Want{status, text, false}; }
Want served() { return Want{}; }

struct Row { const char *name; FusedFacts f; Ask a; Want w; };

const FusedFacts kD = with_actor(handle(false, 7), ActorKind::Discrete, 0.0f), kDNoLimit = with_actor(handle(false, 0), ActorKind::Discrete, 0.0f);
const FusedFacts kDNoCritic = with_actor(handle(false, 7), ActorKind::Discrete, 0.0f, false);
const FusedFacts kB = with_actor(handle(true, 7), ActorKind::Box, 0.5f), kBNoLimit = with_actor(handle(true, 0), ActorKind::Box, 0.5f);
const FusedFacts kBNoCritic = with_actor(handle(true, 7), ActorKind::Box, 0.5f, false), kBFresh = with_actor(handle(true, 7), ActorKind::Box, 0.0f);

#define NEEDS_VALUE "d_rec_boot: V(terminal observation) is recorded beside the values: d_rec_value is null"
#define NO_LIMIT "d_rec_boot: this handle has no time limit (max_episode_steps == 0): no episode is truncated and no row needs a boot"
#define BOOT_ALIGN "d_rec_boot must be 4-byte aligned"
#define NO_CRITIC "d_rec_value: no critic configured (gymnet_vecenv_actor_critic_config)"
#define SRC_VALUE "d_rec_value: values are recorded where the actor chooses (action_source GYMNET_ACTIONS_ACTOR), not "
#define SRC_BOX(what) what ": log-densities and values are recorded where the actor chooses (action_source GYMNET_ACTIONS_ACTOR), not "
#define BOX_ON_VALUE "d_rec_value: this handle's actor chooses Box actions; the fused rollout records values for a Discrete actor (gymnet_vecenv_actor_value_device serves a Box actor)"
#define DISCRETE(what) what ": this handle's actor chooses Discrete actions; a log-density belongs to a Box actor (gymnet_vecenv_rollout_fused_value_device records a Discrete actor's log-probability and value)"
#define SIGMA(what, s) what ": the log-density needs a policy with sigma > 0 and a finite 1 / sigma (gymnet_vecenv_actor_box_set_policy), not " s
#define STALE "the actor's history is stale: reset the actor (or push) before an actor rollout"
#define FRAME_SKIP "the fused actor rollout has no frame skip: run the unfused loop, one decision at a time (actor_act_device, step_repeat_device, actor_push_device)"

const std::vector<Row> kRows = {
    // ---- the Discrete call: each new refusal as the first failure, and served
    {"boot without value", kD, boot_at(actor_rollout(), 0), refused(NEEDS_VALUE)},
    {"boot and logp without value", kD, boot_at(logp_at(actor_rollout(), 0), 0), refused(NEEDS_VALUE)},
    {"no time limit", kDNoLimit, boot_at(value_at(actor_rollout(), 0), 0), refused(NO_LIMIT)},
    {"boot 2 bytes off", kD, boot_at(value_at(actor_rollout(), 0), 2), refused(BOOT_ALIGN)},
    {"boot 1 byte off", kD, boot_at(value_at(actor_rollout(), 0), 1), refused(BOOT_ALIGN)},
    {"served", kD, boot_at(value_at(actor_rollout(), 0), 0), served()},
    {"served with logp, 4 bytes off a line", kD, boot_at(value_at(logp_at(actor_rollout(), 4), 4), 4), served()},
    {"steps 0 with a boot pointer", kD, steps(boot_at(value_at(actor_rollout(), 0), 0), 0), Want{GYMNET_OK, "", true}},
    // ---- every check of the forwarding target applies, with its text
    {"ring source", kD, boot_at(value_at(actor_rollout(GYMNET_ACTIONS_RING), 0), 0), refused(SRC_VALUE "0")},
    {"no actor", handle(false, 7), boot_at(value_at(actor_rollout(), 0), 0), refused("no actor configured (gymnet_vecenv_actor_config)")},
    {"a Box actor through the Discrete call", kB, boot_at(value_at(actor_rollout(), 0), 0), refused(BOX_ON_VALUE)},
    {"no critic", kDNoCritic, boot_at(value_at(actor_rollout(), 0), 0), refused(NO_CRITIC)},
    {"logp 2 bytes off", kD, boot_at(value_at(logp_at(actor_rollout(), 2), 0), 0), refused("d_rec_logp must be 4-byte aligned")},
    {"value 2 bytes off", kD, boot_at(value_at(actor_rollout(), 2), 0), refused("d_rec_value must be 4-byte aligned")},
    // ---- the order
    {"null spec comes first", kD, null_spec(boot_at(actor_rollout(), 2)), refused("spec is null")},
    {"boot without value before the source", kD, boot_at(actor_rollout(GYMNET_ACTIONS_RING), 0), refused(NEEDS_VALUE)},
    {"boot without value before no actor", handle(false, 0), boot_at(actor_rollout(), 2), refused(NEEDS_VALUE)},
    {"the source before the time limit", kDNoLimit, boot_at(value_at(actor_rollout(GYMNET_ACTIONS_SAMPLE), 0), 0), refused(SRC_VALUE "1")},
    {"no critic before the time limit", with_actor(handle(false, 0), ActorKind::Discrete, 0.0f, false), boot_at(value_at(actor_rollout(), 0), 2), refused(NO_CRITIC)},
    {"value's alignment before the time limit", kDNoLimit, boot_at(value_at(actor_rollout(), 2), 2), refused("d_rec_value must be 4-byte aligned")},
    {"the time limit before boot's alignment", kDNoLimit, boot_at(value_at(actor_rollout(), 0), 2), refused(NO_LIMIT)},
    {"boot's alignment before the rollout's own checks", with_actor(handle(false, 7), ActorKind::Discrete, 0.0f, true, false), boot_at(value_at(actor_rollout(), 0), 2), refused(BOOT_ALIGN)},
    // ---- then the rollout's own checks apply
    {"stale history", with_actor(handle(false, 7), ActorKind::Discrete, 0.0f, true, false), boot_at(value_at(actor_rollout(), 0), 0), refused(STALE)},
    {"frame skip", kD, held(boot_at(value_at(actor_rollout(), 0), 0), 1), refused(FRAME_SKIP, GYMNET_ERR_UNSUPPORTED)},
    {"a float64 handle", [] { FusedFacts f = kD; f.f64 = true; return f; }(), boot_at(value_at(actor_rollout(), 0), 0), refused("the fused actor rollout runs float32 handles (float64: act / step / push)", GYMNET_ERR_UNSUPPORTED)},
    // ---- the Box call
    {"box: boot without value", kB, box_boot_at(actor_rollout(), 0), refused(NEEDS_VALUE)},
    {"box: boot and logd without value", kB, box_boot_at(logd_at(actor_rollout(), 0), 0), refused(NEEDS_VALUE)},
    {"box: no time limit", kBNoLimit, box_boot_at(box_value_at(actor_rollout(), 0), 0), refused(NO_LIMIT)},
    {"box: boot 2 bytes off", kB, box_boot_at(box_value_at(logd_at(actor_rollout(), 0), 0), 2), refused(BOOT_ALIGN)},
    {"box: served without logd", kB, box_boot_at(box_value_at(actor_rollout(), 0), 0), served()},
    {"box: served with logd", kB, box_boot_at(box_value_at(logd_at(actor_rollout(), 4), 4), 4), served()},
    {"box: steps 0", kB, steps(box_boot_at(box_value_at(actor_rollout(), 0), 0), 0), Want{GYMNET_OK, "", true}},
    {"box: sampled source", kB, box_boot_at(box_value_at(actor_rollout(GYMNET_ACTIONS_SAMPLE), 0), 0), refused(SRC_BOX("d_rec_value") "1")},
    {"box: sampled source, with logd", kB, box_boot_at(box_value_at(logd_at(actor_rollout(GYMNET_ACTIONS_SAMPLE), 0), 0), 0), refused(SRC_BOX("d_rec_logd") "1")},
    {"box: no actor", handle(true, 7), box_boot_at(box_value_at(actor_rollout(), 0), 0), refused("no actor configured (gymnet_vecenv_actor_box_config)")},
    {"box: a Discrete actor through the Box call", kD, box_boot_at(box_value_at(actor_rollout(), 0), 0), refused(DISCRETE("d_rec_value"))},
    {"box: sigma 0", kBFresh, box_boot_at(box_value_at(actor_rollout(), 0), 0), refused(SIGMA("d_rec_value", "0"))},
    {"box: no critic", kBNoCritic, box_boot_at(box_value_at(actor_rollout(), 0), 0), refused(NO_CRITIC)},
    {"box: logd 2 bytes off", kB, box_boot_at(box_value_at(logd_at(actor_rollout(), 2), 0), 0), refused("d_rec_logd must be 4-byte aligned")},
    {"box: value 2 bytes off", kB, box_boot_at(box_value_at(actor_rollout(), 2), 0), refused("d_rec_value must be 4-byte aligned")},
    {"box: boot without value before the source", kB, box_boot_at(actor_rollout(GYMNET_ACTIONS_RING), 0), refused(NEEDS_VALUE)},
    {"box: sigma before the time limit", with_actor(handle(true, 0), ActorKind::Box, 0.0f), box_boot_at(box_value_at(actor_rollout(), 0), 0), refused(SIGMA("d_rec_value", "0"))},
    {"box: value's alignment before the time limit", kBNoLimit, box_boot_at(box_value_at(actor_rollout(), 2), 2), refused("d_rec_value must be 4-byte aligned")},
    {"box: the time limit before boot's alignment", kBNoLimit, box_boot_at(box_value_at(actor_rollout(), 0), 2), refused(NO_LIMIT)},
    {"box: boot's alignment before the rollout's own checks", with_actor(handle(true, 7), ActorKind::Box, 0.5f, true, false), box_boot_at(box_value_at(actor_rollout(), 0), 2), refused(BOOT_ALIGN)},
    {"box: stale history", with_actor(handle(true, 7), ActorKind::Box, 0.5f, true, false), box_boot_at(box_value_at(actor_rollout(), 0), 0), refused(STALE)},
    {"box: frame skip", kB, held(box_boot_at(box_value_at(actor_rollout(), 0), 0), 1), refused(FRAME_SKIP, GYMNET_ERR_UNSUPPORTED)},
    // ---- requests without a boot pointer: what they were (strings of the two older tables)
    {"old value call on a handle without a time limit", kDNoLimit, value_at(actor_rollout(), 4), served()},
    {"old value call, no critic", kDNoCritic, value_at(actor_rollout(), 0), refused(NO_CRITIC)},
    {"old logp call, 2 bytes off", kD, logp_at(actor_rollout(), 2), refused("d_rec_logp must be 4-byte aligned")},
    {"old value call on a Box actor", kB, value_at(actor_rollout(), 0), refused(BOX_ON_VALUE)},
    {"old box call without a time limit", kBNoLimit, box_value_at(logd_at(actor_rollout(), 0), 0), served()},
    {"old box call, logd alone, no critic", kBNoCritic, logd_at(actor_rollout(), 0), served()},
    {"plain actor rollout", kDNoLimit, actor_rollout(), served()},
    {"plain ring rollout", handle(false, 0), actor_rollout(GYMNET_ACTIONS_RING), served()},
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
    rq.rec_boot = static_cast<float *>(a.rec_boot);
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
    // a served boot request plans what the plain actor rollout of the same handle plans: the record pointers change no field of the plan
    struct Pair { FusedFacts f; Ask a; };
    for (const Pair &p : {Pair{kD, boot_at(value_at(actor_rollout(), 0), 0)}, Pair{kD, boot_at(value_at(logp_at(actor_rollout(), 0), 0), 0)},
                          Pair{kB, box_boot_at(box_value_at(actor_rollout(), 0), 0)}, Pair{kB, box_boot_at(box_value_at(logd_at(actor_rollout(), 0), 0), 0)}}) {
        const FusedOutcome with = plan_fused_rollout(p.f, request(p.a)), plain = plan_fused_rollout(p.f, request(actor_rollout()));
        ++rows;
        if (!(with.status == GYMNET_OK && plain.status == GYMNET_OK && same_plan(with.plan, plain.plan) && with.plan.actor && with.plan.ticks == 8)) {
            ++failed;
            std::printf("FAILED a served boot request's plan differs from the plain rollout's\n");
        }
    }
    // the new fact at its default and at a value: the time limit a handle carries changes nothing for a request without a boot pointer
    for (const Ask &a : {actor_rollout(), value_at(actor_rollout(), 0), value_at(logp_at(actor_rollout(), 2), 0), logp_at(actor_rollout(), 0),
                         box_value_at(logd_at(actor_rollout(), 0), 0), box_value_at(actor_rollout(), 2), logd_at(actor_rollout(), 0), held(actor_rollout(), 1),
                         actor_rollout(GYMNET_ACTIONS_SAMPLE), actor_rollout(GYMNET_ACTIONS_RING)}) {
        for (const ActorKind kind : {ActorKind::Box, ActorKind::Discrete}) {
            for (const bool critic : {false, true}) {
                FusedFacts zero = with_actor(handle(kind == ActorKind::Box, 7), kind, 0.5f, critic), f = zero;
                zero.max_episode_steps = 0;                              // (everything else a time limit implies stays: only the new fact moves)
                const FusedOutcome want = plan_fused_rollout(zero, request(a)), got = plan_fused_rollout(f, request(a));
                ++rows;
                if (!(want.status == got.status && std::strcmp(want.text, got.text) == 0 && same_plan(want.plan, got.plan))) {
                    ++failed;
                    std::printf("FAILED the time limit changes an old request: \"%s\" against \"%s\"\n", got.text, want.text);
                }
            }
        }
    }
    // aggregate initialisations of the parent keep compiling and mean what they meant
    {
        gymnet_rollout_spec sp{};
        const FusedRequest a{&sp}, b{&sp, 0, false, static_cast<float *>(at(LOGP, 0))}, c{&sp, 0, false, nullptr, static_cast<float *>(at(VALUE, 0))};
        ++rows;
        if (!(a.rec_boot == nullptr && b.rec_boot == nullptr && c.rec_boot == nullptr && c.rec_value && !c.box_value && FusedFacts{}.max_episode_steps == 0)) {
            ++failed;
            std::printf("FAILED the appended fields' defaults\n");
        }
    }
    std::printf("%d rows, %d failed\n", rows, failed);
    return failed ? 1 : 0;
}
