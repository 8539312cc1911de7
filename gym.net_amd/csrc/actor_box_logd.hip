// actor_box_logd.hip — the Box actor (actor_box.hip, actor_box_policy.hip) that also records the log-density of every action taken and,
// inside the fused rollout, the critic's value of the input the action was chosen from.  The contract is
// gymnet_vecenv_actor_box_act_logd_device and gymnet_vecenv_rollout_fused_box_logd_device in include/gymnet_amd.h.  With g the greedy
// action after the head (policy_greedy), a the float32 action the lane takes (what d_actions / d_rec_actions receive, after the clamp)
// and sigma the handle's policy's, > 0:
//   inv_sigma = (float)(1.0 / (double)sigma)                                host, once per launch (box_logd_args, rollout_plan.hpp)
//   c         = (float)(-log((double)sigma) - 0.91893853320467274178)       host, once per launch: -ln sigma - ln(2 pi) / 2
//   d    = (a - g) * inv_sigma          float32, each operation rounding on its own
//   h    = -0.5f * d
//   logd = fmaf(h, d, c)
// which is log N(a; g, sigma^2), the density of the unclamped Gaussian at the action taken.  What follows from it:
//   - the noise is added after the head, so a tanh head needs no Jacobian term;
//   - it is recorded for every lane at the stored sigma, whatever explore is and whatever the coin says (as the Discrete logp reports the
//     policy's probability under ("uniform", tau) too): a lane that does not explore has a == g and gets exactly c; under SAMPLE it is the
//     Gaussian policy's density at the uniformly drawn action; it is exactly the behaviour policy's density only at epsilon = 1 under
//     GAUSSIAN, away from the bounds;
//   - where the clamp bit, it is the density at the bound (the point mass there is ignored: the usual PPO treatment);
//   - a NaN g gives a NaN, a d^2 that overflows gives -inf.
// tests/_actor_box_logd_twin.py restates the five lines in NumPy float32 and reproduces the bits.
//
// Act (actor_box_logd_act_kernel): actor_box_policy_act_kernel plus the logd store.  It serves every policy, the default
// ("clamp", "sample") with sigma > 0 included: a request for logd runs this unit whatever the policy.
//
// Fused rollout (actor_box_logd_rollout_kernel): actor_box_policy_rollout_kernel with the log-density's two constants, the critic's
// network and the two record pointers as further arguments — the written-out prologue, rollout_body, one lane per thread, behind a hook
// whose choose() composes the action with policy_choose (actor_box_compose.hpp, the function actor_box_policy.hip runs: actions are the
// same bits with and without the request), stores logd at rec_logd + t * n + i where that pointer is not null, and where rec_value is not
// null loads the input AGAIN, runs the critic over it and stores output 0 at rec_value + t * n + i (one x[64] live at a time, as
// ActorValueHook, actor_value.hip).  Both null checks are wave-uniform branches: one kernel per form.  after() is the shared push:
// bit-identical to steps x (box_act_logd, value, step, push).
//
// Not built: the old names (d_logp, d_rec_logp, d_rec_value alone) lifted for a Box actor, noise before the tanh head (a squashed
// Gaussian with its Jacobian), a learned or per-lane sigma, logd carried through the episode memory.  (V(terminal observation) for
// gymnet_gae_device's boot rows: actor_boot.hip.)
#include "actor_box_compose.hpp"

namespace gymnet {

// (the five lines above, for one lane: box_logd, actor_box_compose.hpp, which actor_boot.hip's rollout runs too)

template <int O>
__global__ __launch_bounds__(256) void actor_box_logd_act_kernel(const ActorNet net, const ActorHist hs, float *__restrict__ actions,
                                                                 float *__restrict__ raw, float *__restrict__ logd, float low, float high, const ActorAct aa,
                                                                 const BoxPolicy pol, const BoxLogd ld) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hs.n) return;
    float r, g;
    const float a = policy_choose<O>(net, hs, hs.slot, i, low, high, pol, coin_threshold(aa.epsilon), aa.seed, aa.lane_offset + (uint64_t)i, aa.tick, r, g);
    actions[i] = a;
    if (raw) raw[i] = r;
    logd[i] = box_logd(a, g, ld);
}

// ActorBoxPolicyHook (actor_box_policy.hip) that records logd and the critic's value.  Both record rows are pinned to SGPRs (lanes.hpp
// wave_uniform), as ActorValueHook's (profiles/kernel_resources_actor_box_logd.txt)
template <class Env>
struct ActorBoxLogdHook {
    static constexpr bool CHOOSES = true;
    static constexpr int S = Env::S, O = Env::O;
    static_assert(std::is_same<typename Env::Real, float>::value && Env::BOX_ACTION, "the Box actor serves float32 Box envs, one lane per thread");
    const ActorNet &net;
    const ActorNet &critic;
    const ActorHist &hs;
    const RolloutArgs &ro;
    const BoxPolicy &pol;
    const BoxLogd &ld;
    float *__restrict__ rec_logd;                                            // [steps][n], or null
    float *__restrict__ rec_value;                                           // [steps][n], or null
    int64_t n;
    uint32_t explore_at_or_below;
    uint64_t lane_offset;
    int32_t newest;

    // gymnet_vecenv_actor_box_act_logd_device(epsilon, action_seed, action_tick0 + t), then gymnet_vecenv_actor_value_device
    __device__ __forceinline__ void choose(int64_t t, int64_t i, float (&act)[1]) const {
        float raw, g;
        const float a = policy_choose<O>(net, hs, newest, i, Env::ACTION_LOW, Env::ACTION_HIGH, pol, explore_at_or_below, ro.action_seed,
                                         lane_offset + (uint64_t)i, ro.action_tick0 + (uint64_t)t, raw, g);
        act[0] = a;
        if (rec_logd) wave_uniform(rec_logd + t * n)[i] = box_logd(a, g, ld);   // a wave-uniform branch
        if (rec_value) {                                                     // and another
            float x[kW];
            load_input<O>(hs, newest, i, x);
            actor_forward(critic, x);
            wave_uniform(rec_value + t * n)[i] = x[0];
        }
    }

    // gymnet_vecenv_actor_push_device (actor_net.hpp)
    __device__ __forceinline__ void after(int64_t, int64_t i, const uint8_t (&done)[1], const float (&s)[S][1], const float (&o)[O][1]) {
        hook_push<Env>(hs, newest, i, done, s, o);
    }
};

// actor_box_policy_rollout_kernel (actor_box_policy.hip) with the log-density's constants, the critic and the record pointers: the same
// prologue (written out, see actor.hip), reset-form choice and launch bounds policy, then rollout_body with the hook above
template <class Env, bool AUTORESET, bool EXTRAS, bool RECORDS>
__global__ __launch_bounds__(256, kActorMinBlocks<EXTRAS>) void actor_box_logd_rollout_kernel(const StepArgs a, const RolloutArgs ro, const ActorNet net,
                                                                                             const ActorHist hs, const BoxPolicy pol, const BoxLogd ld,
                                                                                             const ActorNet critic, float *__restrict__ rec_logd,
                                                                                             float *__restrict__ rec_value) {
    constexpr bool RESETF = Env::OBS_ALIASES_STATE && AUTORESET;         // the wave-compacted reset where the env has it (MountainCarContinuous)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    ResetScratch<Env> *sc = nullptr;
    if constexpr (RESETF) {
        __shared__ ResetScratch<Env> scratch[256 / 64];
        sc = &scratch[threadIdx.x >> 6];
    }
    EpisodeStage *stage = nullptr;
    if constexpr (EXTRAS && RECORDS) {
        __shared__ EpisodeStage stages[256 / 64];
        stage = &stages[threadIdx.x >> 6];
    }
    const uint64_t tick0 = a.tick2[a.parity];
    if (blockIdx.x == 0 && threadIdx.x == 0) a.tick2[a.parity ^ 1] = tick0 + (uint64_t)ro.steps;
    if constexpr (EXTRAS) {
        if (blockIdx.x == 0 && a.done_count2) {
            // (not vectorised: see actor_box_rollout_kernel)
#pragma clang loop vectorize(disable) interleave(disable)
            for (int sh = threadIdx.x; sh < kShards; sh += blockDim.x) a.done_count2[(a.cparity ^ 1) * (kShards * kCountStride) + sh * kCountStride] = 0u;
        }
    }
    // every lane of the thread is in range past this line (no GUARD form), and the active lanes of the last wave are a prefix (the
    // wave-level helpers rely on it)
    if (i >= a.n) return;
    const ActorBoxLogdHook<Env> hook{net, critic, hs, ro, pol, ld, rec_logd, rec_value, a.n, coin_threshold(ro.epsilon), a.lane_offset, hs.slot};
    rollout_body<Env, 1, AUTORESET, false, EXTRAS, false, RESETF ? 1 : 0, RECORDS ? 1 : 0>(a, ro, i, tick0, sc, stage, hook);
}

template <class Env>
static hipError_t launch_logd_rollout_env(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r, float *rec_logd, float *rec_value) {
    const auto k = pick_rollout_form(h->autoreset, h->extras, records, [](auto ar, auto ex, auto rec) { return actor_box_logd_rollout_kernel<Env, ar, ex, rec>; });
    const Actor &ac = *h->actor;
    hipLaunchKernelGGL(k, lane_grid(a.n), dim3(256), 0, h->stream, a, r, ac.net, ac.hist, box_policy(ac), box_logd_args(ac.sigma), ac.critic, rec_logd, rec_value);
    return hipGetLastError();
}

// actor.hip's router sends a Box actor's rollout asked for through gymnet_vecenv_rollout_fused_box_logd_device here, under any policy,
// with either record pointer or both
hipError_t actor_box_logd_rollout_launch(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r, float *rec_logd, float *rec_value) {
    const Actor &ac = *h->actor;
    // (the plan has refused both: rollout_plan.hpp box_record_pointers)
    if (!box_sigma_ok(ac.sigma) || (rec_value && !ac.has_critic())) return hipErrorInvalidValue;
    switch (h->cfg.env_id) {
        case GYMNET_ENV_PENDULUM: return launch_logd_rollout_env<Pendulum>(h, records, a, r, rec_logd, rec_value);
        case GYMNET_ENV_MOUNTAINCAR_CONTINUOUS: return launch_logd_rollout_env<MountainCarContinuous>(h, records, a, r, rec_logd, rec_value);
        default: return hipErrorInvalidValue;
    }
}

namespace {

hipError_t launch_box_logd_act(const ActorNet &net, const ActorHist &hs, float *actions, float *raw, float *logd, float low, float high, const ActorAct &aa,
                               const BoxPolicy &pol, const BoxLogd &ld, hipStream_t st) {
    if (hs.n <= 0) return hipSuccess;
    switch (hs.obs_dim) {
        case 2: hipLaunchKernelGGL(actor_box_logd_act_kernel<2>, lane_grid(hs.n), dim3(256), 0, st, net, hs, actions, raw, logd, low, high, aa, pol, ld); break;
        case 3: hipLaunchKernelGGL(actor_box_logd_act_kernel<3>, lane_grid(hs.n), dim3(256), 0, st, net, hs, actions, raw, logd, low, high, aa, pol, ld); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

}  // namespace gymnet

using namespace gymnet;

extern "C" {

int gymnet_vecenv_actor_box_act_logd_device(gymnet_vecenv *h, float *d_actions, float *d_raw, float *d_logd, float epsilon, uint64_t seed, uint64_t tick) {
    if (!d_logd) return gymnet_vecenv_actor_box_act_device(h, d_actions, d_raw, epsilon, seed, tick);
    return guarded([&]() -> int {
    ENTER(h);
    ActorAct aa;
    ST_TRY(actor_act_enter(h, true, "this handle's actor chooses Discrete actions: a log-density belongs to a Box actor (gymnet_vecenv_actor_act_logp_device)",
                           d_actions, nullptr, epsilon, seed, tick, aa));
    if (!aligned_to(d_logd, 4)) return fail(h, GYMNET_ERR_INVALID_ARG, "d_logd must be 4-byte aligned");
    const Actor &ac = *h->actor;
    if (!box_sigma_ok(ac.sigma)) return fail(h, GYMNET_ERR_INVALID_ARG, kBadSigmaFormat, "d_logd", (double)ac.sigma);
    HIP_TRY(h, launch_box_logd_act(ac.net, ac.hist, d_actions, d_raw, d_logd, h->desc->action_low, h->desc->action_high, aa, box_policy(ac),
                                   box_logd_args(ac.sigma), h->stream));
    return GYMNET_OK;
    });
}

}  // extern "C"
