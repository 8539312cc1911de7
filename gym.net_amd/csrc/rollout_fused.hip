// rollout_fused.hip — the fused rollout's host side: gymnet_vecenv_rollout_fused_device and its _ex / _logp / _value / _box_logd / _value_boot / _box_boot siblings, and the
// handle's episode-segment block (h->ep).  Host code only; this unit holds no kernel.  What a call will do — every refusal, the lane width,
// the segment block, the ticks — is decided by rollout_plan.hpp's pure function; here the facts are gathered, the plan is carried out.
#include <hip/hip_runtime.h>

#include "handle.hpp"

using namespace gymnet;

namespace {

// the handle's segment block as the plan wants it: the handle's own where it holds the request, else a larger one in its place
int ensure_episode_segments(gymnet_vecenv *h, const FusedPlan &plan) {
    if (!plan.grow) return GYMNET_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));          // a previous rollout's gather may still read the old segments
    if (h->ep.d) (void)hipFree(h->ep.d);
    h->ep = EpisodeBlock{};
    void *q = nullptr;
    const size_t bytes = plan.segments.bytes();
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail(h, GYMNET_ERR_OOM, "hipMalloc(%zu bytes) for the rollout's episode records failed: %s", bytes, hipGetErrorString(e));
    h->ep = EpisodeBlock{q, plan.segments};
    return GYMNET_OK;
}

template <class R>
int rollout_fused_typed(gymnet_vecenv *h, const FusedRequest &rq, const FusedPlan &plan) {
    const gymnet_rollout_spec &sp = *rq.spec;
    const bool episodes = plan.episodes;
    LaunchCfg cfg = h->lcfg;
    cfg.vec = plan.vec;
    const StepArgsT<R> a = make_step_args<R>(h, sp.d_actions);
    RolloutArgsT<R> r{};
    r.steps = sp.steps; r.action_stride = sp.action_stride; r.ring = sp.ring;
    r.rec_obs = static_cast<R *>(sp.d_rec_obs); r.rec_reward = sp.d_rec_reward; r.rec_done = sp.d_rec_done;
    r.rec_action = sp.d_rec_actions;
    r.action_source = sp.action_source; r.epsilon = sp.epsilon; r.action_seed = sp.action_seed; r.action_tick0 = sp.action_tick0;
    if (episodes) {
        char *seg = static_cast<char *>(h->ep.d);
        const EpisodeSegments &lay = h->ep.seg;
        r.ep_t = reinterpret_cast<int32_t *>(seg + lay.offset(0)); r.ep_lane = reinterpret_cast<int32_t *>(seg + lay.offset(1));
        r.ep_ret = h->d_ep_ret ? reinterpret_cast<float *>(seg + lay.offset(2)) : nullptr;
        r.ep_len = h->d_ep_ret ? reinterpret_cast<int32_t *>(seg + lay.offset(3)) : nullptr;
        r.ep_count = reinterpret_cast<uint32_t *>(seg + lay.counters_offset());
        r.ep_cap = lay.cap;
        r.ov_cap = plan.ov_cap;
        r.records_no_overflow = (sp.record_flags & GYMNET_RECORDS_NO_OVERFLOW) ? 1 : 0;
        // the kShards + 1 counters, zeroed on the stream by a kernel of our own
        HIP_TRY(h, launch_fill_i32(reinterpret_cast<int32_t *>(r.ep_count), 0, (int64_t)(kShards + 1) * kCountStride, h->stream));
    }
    if (rq.held > 0) {
        HIP_TRY(h, repeat_rollout_launch(h, a, r, rq.held + 1));
    } else if constexpr (sizeof(R) == 4) {
        if (plan.actor) {
            HIP_TRY(h, actor_rollout_launch(h, episodes, a, r, rq));
        } else {
            HIP_TRY(h, launchers<R>(h).rollout(h->autoreset, h->extras, a, r, cfg, h->stream));
        }
    } else {
        HIP_TRY(h, launchers<R>(h).rollout(h->autoreset, h->extras, a, r, cfg, h->stream));
    }
    if (episodes) {
        EpisodeGatherArgs g{};
        g.counts = r.ep_count; g.cap = r.ep_cap;
        g.ep_t = r.ep_t; g.ep_lane = r.ep_lane; g.ep_ret = r.ep_ret; g.ep_len = r.ep_len;
        g.ov_cap = r.ov_cap;
        g.out_t = sp.d_ep_step; g.out_lane = sp.d_ep_lane; g.out_ret = sp.d_ep_return; g.out_len = sp.d_ep_length;
        g.out_capacity = sp.ep_capacity; g.out_count = sp.d_ep_count;
        HIP_TRY(h, launch_gather_episodes(g, h->stream));
    }
    h->last_cparity = a.cparity;          // the done list (if any) describes the rollout's last step
    return GYMNET_OK;
}

FusedFacts fused_facts(const gymnet_vecenv *h) {
    FusedFacts f;
    f.n = h->n; f.sstride = h->sstride;
    f.f64 = h->f64; f.alias = h->desc->alias; f.box_action = h->desc->box_action;
    f.extras = h->extras; f.ep_stats = h->d_ep_ret != nullptr;
    f.validate_actions = (h->cfg.flags & GYMNET_FLAG_VALIDATE_ACTIONS) != 0;
    f.vec = h->lcfg.vec;
    f.actor = actor_facts(h);
    f.has_segments = h->ep.d != nullptr; f.segments = h->ep.seg;
    f.max_episode_steps = h->cfg.max_episode_steps;
    return f;
}

}  // namespace

namespace gymnet {

int rollout_fused_entered(gymnet_vecenv *h, const FusedRequest &rq) {
    const FusedOutcome out = plan_fused_rollout(fused_facts(h), rq);
    if (out.status != GYMNET_OK) return fail(h, out.status, "%s", out.text);
    const FusedPlan &plan = out.plan;
    const gymnet_rollout_spec &sp = *rq.spec;
    if (plan.zero_steps) {
        if (plan.episodes) HIP_TRY(h, hipMemsetAsync(sp.d_ep_count, 0, 2 * sizeof(uint32_t), h->stream));
        return GYMNET_OK;
    }
    if (plan.episodes) ST_TRY(ensure_episode_segments(h, plan));
    ST_TRY(h->f64 ? rollout_fused_typed<double>(h, rq, plan) : rollout_fused_typed<float>(h, rq, plan));
    swap_buffers(h);                     // DOUBLE_BUFFER: the launch read one buffer and wrote the other, once
    h->tick += plan.ticks;
    h->held_ticks += plan.held_ticks;
    h->tslot ^= 1;                       // one launch: it read one half of d_tick2 and wrote the other
    h->step_launches += 1;
    h->lane_steps += plan.ticks * (uint64_t)h->n;      // slots: the host does not know which sub-steps found their lane idle
    if (plan.actor) actor_rollout_done(h, sp.steps);
    return GYMNET_OK;
}

}  // namespace gymnet

extern "C" {

int gymnet_vecenv_rollout_fused_device(gymnet_vecenv *h, const void *d_actions, int64_t steps, int64_t action_stride,
                                       int64_t ring, const gymnet_rollout_buffers *rec) {
    gymnet_rollout_spec spec{};
    spec.struct_size = sizeof spec;
    spec.action_source = GYMNET_ACTIONS_RING;
    spec.d_actions = d_actions; spec.steps = steps; spec.action_stride = action_stride; spec.ring = ring;
    if (rec) { spec.d_rec_obs = rec->d_obs; spec.d_rec_reward = rec->d_reward; spec.d_rec_done = rec->d_done; }
    return gymnet_vecenv_rollout_fused_ex_device(h, &spec);
}

int gymnet_vecenv_rollout_fused_ex_device(gymnet_vecenv *h, const gymnet_rollout_spec *spec) {
    return guarded([&]() -> int {
    ENTER(h);
    return rollout_fused_entered(h, FusedRequest{spec});
    });
}

// the null-pointer forwarding chain: value -> logp -> ex.  The record pointers' own checks are the plan's (they run behind the spec's
// null / struct_size test and before the rollout's own)
int gymnet_vecenv_rollout_fused_logp_device(gymnet_vecenv *h, const gymnet_rollout_spec *spec, float *d_rec_logp) {
    if (!d_rec_logp) return gymnet_vecenv_rollout_fused_ex_device(h, spec);
    return guarded([&]() -> int {
    ENTER(h);
    return rollout_fused_entered(h, FusedRequest{spec, 0, false, d_rec_logp});
    });
}

int gymnet_vecenv_rollout_fused_value_device(gymnet_vecenv *h, const gymnet_rollout_spec *spec, float *d_rec_logp, float *d_rec_value) {
    if (!d_rec_value) return gymnet_vecenv_rollout_fused_logp_device(h, spec, d_rec_logp);
    return guarded([&]() -> int {
    ENTER(h);
    return rollout_fused_entered(h, FusedRequest{spec, 0, false, d_rec_logp, d_rec_value});
    });
}

// the Box actor's pair (actor_box_logd.hip): either pointer or both; neither: the plain call.  Their checks are the plan's too
// (box_record_pointers)
int gymnet_vecenv_rollout_fused_box_logd_device(gymnet_vecenv *h, const gymnet_rollout_spec *spec, float *d_rec_logd, float *d_rec_value) {
    if (!d_rec_logd && !d_rec_value) return gymnet_vecenv_rollout_fused_ex_device(h, spec);
    return guarded([&]() -> int {
    ENTER(h);
    FusedRequest rq{spec};
    rq.rec_value = d_rec_value; rq.rec_logd = d_rec_logd; rq.box_value = d_rec_value != nullptr;
    return rollout_fused_entered(h, rq);
    });
}

// the two calls that also record V(terminal observation) on time-limit rows (actor_boot.hip): without a boot pointer, the calls above
int gymnet_vecenv_rollout_fused_value_boot_device(gymnet_vecenv *h, const gymnet_rollout_spec *spec, float *d_rec_logp, float *d_rec_value, float *d_rec_boot) {
    if (!d_rec_boot) return gymnet_vecenv_rollout_fused_value_device(h, spec, d_rec_logp, d_rec_value);
    return guarded([&]() -> int {
    ENTER(h);
    FusedRequest rq{spec, 0, false, d_rec_logp, d_rec_value};
    rq.rec_boot = d_rec_boot;
    return rollout_fused_entered(h, rq);
    });
}

int gymnet_vecenv_rollout_fused_box_boot_device(gymnet_vecenv *h, const gymnet_rollout_spec *spec, float *d_rec_logd, float *d_rec_value, float *d_rec_boot) {
    if (!d_rec_boot) return gymnet_vecenv_rollout_fused_box_logd_device(h, spec, d_rec_logd, d_rec_value);
    return guarded([&]() -> int {
    ENTER(h);
    FusedRequest rq{spec};
    rq.rec_value = d_rec_value; rq.rec_logd = d_rec_logd; rq.box_value = true; rq.rec_boot = d_rec_boot;
    return rollout_fused_entered(h, rq);
    });
}

}  // extern "C"
