// actor_boot.hip — V(terminal observation) on time-limit rows: what gymnet_gae_device's d_boot takes, so that a truncated episode
// bootstraps from the critic's value of the state it stopped in and not from zero.  The contract is gymnet_vecenv_actor_boot_device and
// the two gymnet_vecenv_rollout_fused_*_boot_device calls in include/gymnet_amd.h.  For a lane with this step's done byte d, history
// depth S, ring o_{p-S+1} .. o_p (the input the action was chosen from) and terminal observation o_term (the post-step observation
// before any reset):
//   boot = (d & 2) ? critic(o_{p-S+2}, .., o_p, (float)o_term)[0] : +0.0f
// The critic is actor_forward (actor_net.hpp) over its packed weights: the fmaf chain actor_value_device runs, over the input that call
// would read had o_term been pushed with a done byte of 0.  No new arithmetic: tests/_actor_twin.py's forward reproduces the bits up to
// the sign of a zero (twin.same).  d == 3 gets the value too (gymnet_gae_device lets "terminated" win and ignores it); rows without bit 1
// get +0.0f.
//
// Stand-alone (actor_boot_kernel): one lane per thread, as actor_value_kernel.  The done bytes and o_term come from memory: on an
// AUTORESET handle the dense FINAL_OBS rows (the step kernel wrote them in the step that set the done byte), otherwise the handle's
// current observation; cast to float32 as actor_push_kernel casts, so float64 handles are served as Value() serves them.
//
// Fused rollout (actor_value_boot_rollout_kernel, actor_box_boot_rollout_kernel): actor_value_rollout_kernel / actor_box_logd_rollout_
// kernel with rec_boot as a further argument, behind hooks whose choose() and after() are ActorValueHook's / ActorBoxLogdHook's and
// which declare BOOTS: rollout_body (step_kernels.hpp) then calls terminal() between the step's rec_* scalar stores and the fused reset,
// where o_term is still in the lane's registers and the ring still holds the S - 1 observations before it (after() has not pushed yet).
// terminal() ballots (d & 2) and skips the whole evaluation when no lane of the wave is truncated — at a 500-step limit almost every
// wave skips almost every step —, otherwise the truncated lanes load ring rows 1 .. S-1, append o_term as hook_push picks it and run the
// critic under the execution mask; every lane stores its boot at rec_boot + t * n + i.  FINAL_OBS is not needed.  Only the bookkeeping
// forms exist (a time limit needs EPISODE_STATS): AUTORESET x RECORDS for each of the five float32 envs, 20 kernels.
//
// actor_forward is inlined a third time (behind the ballot, so the hot route jumps over it): a shared non-inlined form would pass
// x[64] through scratch in every form and on every call, the two hot ones included; code bytes and registers of all 20 forms are in
// profiles/kernel_resources_actor_boot.txt.
//
// Not built: boot carried through the episode memory's rows, frame skip inside the fused actor rollout, any gradient.
#include "actor_box_compose.hpp"
#include "actor_compose_logp.hpp"

namespace gymnet {

namespace {

// the critic's input for a boot row: ring rows 1 .. S-1 of the window whose newest slot is `newest`, then v (the terminal observation)
template <int O>
__device__ __forceinline__ void load_boot_input(const ActorHist &hs, int32_t newest, int64_t i, const float (&v)[O], float (&x)[kW]) {
#pragma unroll
    for (int q = 0; q < kW / O; ++q) {
        int32_t row = 0;
        if (q + 1 < hs.history) row = ring_row(newest, q + 1, hs.history);   // wave-uniform
#pragma unroll
        for (int k = 0; k < O; ++k)
            x[q * O + k] = q + 1 < hs.history ? hs.hist[((int64_t)row * O + k) * hs.stride + i] : (q + 1 == hs.history ? v[k] : 0.0f);
    }
#pragma unroll
    for (int i2 = (kW / O) * O; i2 < kW; ++i2) x[i2] = 0.0f;
}

// one lane's boot given its done byte and terminal observation; the evaluation is skipped by a wave that holds no truncated lane
template <int O>
__device__ __forceinline__ float boot_value(const ActorNet &critic, const ActorHist &hs, int32_t newest, int64_t i, uint8_t done, const float (&v)[O]) {
    const bool trunc = (done & 2) != 0;
    float boot = 0.0f;
    if (__ballot(trunc)) {                                                   // wave-uniform
        if (trunc) {
            float x[kW];
            load_boot_input<O>(hs, newest, i, v, x);
            actor_forward(critic, x);
            boot = x[0];
        }
    }
    return boot;
}

// the `terminal` third of rollout_body's hook, one lane per thread: the observation as hook_push picks it, the row pinned as the
// sibling hooks pin theirs
template <class Env>
__device__ __forceinline__ void hook_boot(const ActorNet &critic, const ActorHist &hs, int32_t newest, float *__restrict__ rec_boot, int64_t t, int64_t n,
                                          int64_t i, const uint8_t (&done)[1], const float (&s)[Env::S][1], const float (&o)[Env::O][1]) {
    constexpr int S = Env::S, O = Env::O;
    float v[O];
#pragma unroll
    for (int k = 0; k < O; ++k) v[k] = Env::OBS_ALIASES_STATE ? s[k < S ? k : 0][0] : o[k][0];
    wave_uniform(rec_boot + t * n)[i] = boot_value<O>(critic, hs, newest, i, done[0], v);
}

}  // namespace

template <class R, int O>
__global__ __launch_bounds__(256) void actor_boot_kernel(const ActorNet critic, const ActorHist hs, const R *__restrict__ obs, int64_t obs_stride,
                                                         const uint8_t *__restrict__ done, float *__restrict__ boot) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hs.n) return;
    const uint8_t d = done[i];
    float v[O];
#pragma unroll
    for (int k = 0; k < O; ++k) v[k] = (d & 2) ? (float)obs[k * obs_stride + i] : 0.0f;
    boot[i] = boot_value<O>(critic, hs, hs.slot, i, d, v);
}

// ActorValueHook (actor_value.hip) with terminal(): choose() and after() are that hook's, line for line
template <class Env>
struct ActorValueBootHook {
    static constexpr bool CHOOSES = true, BOOTS = true;
    static constexpr int S = Env::S, O = Env::O;
    static_assert(std::is_same<typename Env::Real, float>::value && !Env::BOX_ACTION, "the actor serves float32 Discrete envs, one lane per thread");
    const ActorNet &net;
    const ActorNet &critic;
    const ActorHist &hs;
    const RolloutArgs &ro;
    const ActorExplore &ex;
    float *__restrict__ rec_logp;                                            // [steps][n], or null
    float *__restrict__ rec_value;                                           // [steps][n]
    float *__restrict__ rec_boot;                                            // [steps][n]
    int64_t n;
    uint32_t explore_at_or_below;
    uint64_t lane_offset;
    int32_t newest;

    __device__ __forceinline__ void choose(int64_t t, int64_t i, int32_t (&act)[1]) const {
        float x[kW];
        load_input<O>(hs, newest, i, x);
        actor_forward(net, x);
        float lp;
        act[0] = compose_one_logp(x, net.action_n, ex, explore_at_or_below, ro.action_seed, lane_offset + (uint64_t)i, ro.action_tick0 + (uint64_t)t, lp);
        if (rec_logp) wave_uniform(rec_logp + t * n)[i] = lp;                // a wave-uniform branch
        load_input<O>(hs, newest, i, x);
        actor_forward(critic, x);
        wave_uniform(rec_value + t * n)[i] = x[0];
    }

    // gymnet_vecenv_actor_boot_device, with the done byte and the terminal observation taken from the rollout's registers
    __device__ __forceinline__ void terminal(int64_t t, int64_t i, const uint8_t (&done)[1], const float (&s)[S][1], const float (&o)[O][1]) const {
        hook_boot<Env>(critic, hs, newest, rec_boot, t, n, i, done, s, o);
    }

    // gymnet_vecenv_actor_push_device (actor_net.hpp)
    __device__ __forceinline__ void after(int64_t, int64_t i, const uint8_t (&done)[1], const float (&s)[S][1], const float (&o)[O][1]) {
        hook_push<Env>(hs, newest, i, done, s, o);
    }
};

// ActorBoxLogdHook (actor_box_logd.hip) with terminal(); rec_value is never null here (the plan: a boot needs the values)
template <class Env>
struct ActorBoxBootHook {
    static constexpr bool CHOOSES = true, BOOTS = true;
    static constexpr int S = Env::S, O = Env::O;
    static_assert(std::is_same<typename Env::Real, float>::value && Env::BOX_ACTION, "the Box actor serves float32 Box envs, one lane per thread");
    const ActorNet &net;
    const ActorNet &critic;
    const ActorHist &hs;
    const RolloutArgs &ro;
    const BoxPolicy &pol;
    const BoxLogd &ld;
    float *__restrict__ rec_logd;                                            // [steps][n], or null
    float *__restrict__ rec_value;                                           // [steps][n]
    float *__restrict__ rec_boot;                                            // [steps][n]
    int64_t n;
    uint32_t explore_at_or_below;
    uint64_t lane_offset;
    int32_t newest;

    __device__ __forceinline__ void choose(int64_t t, int64_t i, float (&act)[1]) const {
        float raw, g;
        const float a = policy_choose<O>(net, hs, newest, i, Env::ACTION_LOW, Env::ACTION_HIGH, pol, explore_at_or_below, ro.action_seed,
                                         lane_offset + (uint64_t)i, ro.action_tick0 + (uint64_t)t, raw, g);
        act[0] = a;
        if (rec_logd) wave_uniform(rec_logd + t * n)[i] = box_logd(a, g, ld);   // a wave-uniform branch
        float x[kW];
        load_input<O>(hs, newest, i, x);
        actor_forward(critic, x);
        wave_uniform(rec_value + t * n)[i] = x[0];
    }

    __device__ __forceinline__ void terminal(int64_t t, int64_t i, const uint8_t (&done)[1], const float (&s)[S][1], const float (&o)[O][1]) const {
        hook_boot<Env>(critic, hs, newest, rec_boot, t, n, i, done, s, o);
    }

    __device__ __forceinline__ void after(int64_t, int64_t i, const uint8_t (&done)[1], const float (&s)[S][1], const float (&o)[O][1]) {
        hook_push<Env>(hs, newest, i, done, s, o);
    }
};

// actor_value_rollout_kernel (actor_value.hip) with the boot pointer: the same prologue (written out, see actor.hip) and reset-form
// choice, bookkeeping forms only, then rollout_body with the hook above
template <class Env, bool AUTORESET, bool RECORDS>
__global__ __launch_bounds__(256, kActorMinBlocks<true>) void actor_value_boot_rollout_kernel(const StepArgs a, const RolloutArgs ro, const ActorNet net,
                                                                                             const ActorHist hs, const ActorExplore ex, const ActorNet critic,
                                                                                             float *__restrict__ rec_logp, float *__restrict__ rec_value,
                                                                                             float *__restrict__ rec_boot) {
    constexpr bool RESETF = Env::OBS_ALIASES_STATE && AUTORESET;         // the wave-compacted reset where the env has it
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    ResetScratch<Env> *sc = nullptr;
    if constexpr (RESETF) {
        __shared__ ResetScratch<Env> scratch[256 / 64];
        sc = &scratch[threadIdx.x >> 6];
    }
    EpisodeStage *stage = nullptr;
    if constexpr (RECORDS) {
        __shared__ EpisodeStage stages[256 / 64];
        stage = &stages[threadIdx.x >> 6];
    }
    const uint64_t tick0 = a.tick2[a.parity];
    if (blockIdx.x == 0 && threadIdx.x == 0) a.tick2[a.parity ^ 1] = tick0 + (uint64_t)ro.steps;
    if (blockIdx.x == 0 && a.done_count2)
        for (int sh = threadIdx.x; sh < kShards; sh += blockDim.x) a.done_count2[(a.cparity ^ 1) * (kShards * kCountStride) + sh * kCountStride] = 0u;
    // every lane of the thread is in range past this line (no GUARD form), and the active lanes of the last wave are a prefix (the
    // wave-level helpers rely on it)
    if (i >= a.n) return;
    const ActorValueBootHook<Env> hook{net, critic, hs, ro, ex, rec_logp, rec_value, rec_boot, a.n, coin_threshold(ro.epsilon), a.lane_offset, hs.slot};
    rollout_body<Env, 1, AUTORESET, false, true, false, RESETF ? 1 : 0, RECORDS ? 1 : 0>(a, ro, i, tick0, sc, stage, hook);
}

// actor_box_logd_rollout_kernel (actor_box_logd.hip) with the boot pointer, bookkeeping forms only
template <class Env, bool AUTORESET, bool RECORDS>
__global__ __launch_bounds__(256, kActorMinBlocks<true>) void actor_box_boot_rollout_kernel(const StepArgs a, const RolloutArgs ro, const ActorNet net,
                                                                                           const ActorHist hs, const BoxPolicy pol, const BoxLogd ld,
                                                                                           const ActorNet critic, float *__restrict__ rec_logd,
                                                                                           float *__restrict__ rec_value, float *__restrict__ rec_boot) {
    constexpr bool RESETF = Env::OBS_ALIASES_STATE && AUTORESET;         // the wave-compacted reset where the env has it (MountainCarContinuous)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    ResetScratch<Env> *sc = nullptr;
    if constexpr (RESETF) {
        __shared__ ResetScratch<Env> scratch[256 / 64];
        sc = &scratch[threadIdx.x >> 6];
    }
    EpisodeStage *stage = nullptr;
    if constexpr (RECORDS) {
        __shared__ EpisodeStage stages[256 / 64];
        stage = &stages[threadIdx.x >> 6];
    }
    const uint64_t tick0 = a.tick2[a.parity];
    if (blockIdx.x == 0 && threadIdx.x == 0) a.tick2[a.parity ^ 1] = tick0 + (uint64_t)ro.steps;
    if (blockIdx.x == 0 && a.done_count2) {
        // (not vectorised: see actor_box_rollout_kernel)
#pragma clang loop vectorize(disable) interleave(disable)
        for (int sh = threadIdx.x; sh < kShards; sh += blockDim.x) a.done_count2[(a.cparity ^ 1) * (kShards * kCountStride) + sh * kCountStride] = 0u;
    }
    if (i >= a.n) return;
    const ActorBoxBootHook<Env> hook{net, critic, hs, ro, pol, ld, rec_logd, rec_value, rec_boot, a.n, coin_threshold(ro.epsilon), a.lane_offset, hs.slot};
    rollout_body<Env, 1, AUTORESET, false, true, false, RESETF ? 1 : 0, RECORDS ? 1 : 0>(a, ro, i, tick0, sc, stage, hook);
}

namespace {

// the two run-time switches of a bookkeeping form as compile-time ones
template <class F>
auto pick_boot_form(bool autoreset, bool records, F f) {
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    if (autoreset) return records ? f(yes, yes) : f(yes, no);
    return records ? f(no, yes) : f(no, no);
}

template <class Env>
hipError_t launch_value_boot_env(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r, float *rec_logp, float *rec_value, float *rec_boot) {
    const auto k = pick_boot_form(h->autoreset, records, [](auto ar, auto rec) { return actor_value_boot_rollout_kernel<Env, ar, rec>; });
    const Actor &ac = *h->actor;
    hipLaunchKernelGGL(k, lane_grid(a.n), dim3(256), 0, h->stream, a, r, ac.net, ac.hist, actor_explore(ac), ac.critic, rec_logp, rec_value, rec_boot);
    return hipGetLastError();
}

template <class Env>
hipError_t launch_box_boot_env(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r, float *rec_logd, float *rec_value, float *rec_boot) {
    const auto k = pick_boot_form(h->autoreset, records, [](auto ar, auto rec) { return actor_box_boot_rollout_kernel<Env, ar, rec>; });
    const Actor &ac = *h->actor;
    hipLaunchKernelGGL(k, lane_grid(a.n), dim3(256), 0, h->stream, a, r, ac.net, ac.hist, box_policy(ac), box_logd_args(ac.sigma), ac.critic, rec_logd, rec_value,
                       rec_boot);
    return hipGetLastError();
}

template <class R>
hipError_t launch_boot_typed(const ActorNet &critic, const ActorHist &hs, const R *obs, int64_t obs_stride, const uint8_t *done, float *boot, hipStream_t st) {
    switch (hs.obs_dim) {
        case 2: hipLaunchKernelGGL((actor_boot_kernel<R, 2>), lane_grid(hs.n), dim3(256), 0, st, critic, hs, obs, obs_stride, done, boot); break;
        case 3:                                       // Pendulum: float32 only
            if constexpr (sizeof(R) == 4) { hipLaunchKernelGGL((actor_boot_kernel<R, 3>), lane_grid(hs.n), dim3(256), 0, st, critic, hs, obs, obs_stride, done, boot); break; }
            else return hipErrorInvalidValue;
        case 4: hipLaunchKernelGGL((actor_boot_kernel<R, 4>), lane_grid(hs.n), dim3(256), 0, st, critic, hs, obs, obs_stride, done, boot); break;
        case 6: hipLaunchKernelGGL((actor_boot_kernel<R, 6>), lane_grid(hs.n), dim3(256), 0, st, critic, hs, obs, obs_stride, done, boot); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

// actor.hip's router sends a rollout with a boot pointer here: a Discrete actor's (rec_logp may be null) ...
hipError_t actor_value_boot_rollout_launch(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r, float *rec_logp, float *rec_value,
                                           float *rec_boot) {
    // (the plan has refused all three: rollout_plan.hpp record_pointers; a time limit implies the bookkeeping forms)
    if (!h->actor->has_critic() || !rec_value || !h->extras) return hipErrorInvalidValue;
    switch (h->cfg.env_id) {
        case GYMNET_ENV_CARTPOLE: return launch_value_boot_env<CartPole>(h, records, a, r, rec_logp, rec_value, rec_boot);
        case GYMNET_ENV_MOUNTAINCAR: return launch_value_boot_env<MountainCar>(h, records, a, r, rec_logp, rec_value, rec_boot);
        case GYMNET_ENV_ACROBOT: return launch_value_boot_env<Acrobot>(h, records, a, r, rec_logp, rec_value, rec_boot);
        default: return hipErrorInvalidValue;
    }
}

// ... and a Box actor's (rec_logd may be null)
hipError_t actor_box_boot_rollout_launch(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r, float *rec_logd, float *rec_value,
                                         float *rec_boot) {
    const Actor &ac = *h->actor;
    // (the plan has refused all four: rollout_plan.hpp box_record_pointers)
    if (!box_sigma_ok(ac.sigma) || !ac.has_critic() || !rec_value || !h->extras) return hipErrorInvalidValue;
    switch (h->cfg.env_id) {
        case GYMNET_ENV_PENDULUM: return launch_box_boot_env<Pendulum>(h, records, a, r, rec_logd, rec_value, rec_boot);
        case GYMNET_ENV_MOUNTAINCAR_CONTINUOUS: return launch_box_boot_env<MountainCarContinuous>(h, records, a, r, rec_logd, rec_value, rec_boot);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace gymnet

using namespace gymnet;

extern "C" {

int gymnet_vecenv_actor_boot_device(gymnet_vecenv *h, float *d_boot) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_actor(h));
    const Actor &ac = *h->actor;
    if (!ac.has_critic()) return fail(h, GYMNET_ERR_INVALID_ARG, "no critic configured (gymnet_vecenv_actor_critic_config)");
    if (!d_boot) return fail(h, GYMNET_ERR_INVALID_ARG, "d_boot is null");
    if (!aligned_to(d_boot, 4)) return fail(h, GYMNET_ERR_INVALID_ARG, "d_boot must be 4-byte aligned");
    if (!(since(h, ac.last) == StepMark{1, 1}))
        return fail(h, GYMNET_ERR_INVALID_ARG, "an actor boot needs exactly one vector step since the last actor config, reset or push: call it after the "
                    "step and before gymnet_vecenv_actor_push_device (%llu steps, %llu step launches, %llu reset / seed / set_tick / set_state calls)",
                    (unsigned long long)since(h, ac.last).tick, (unsigned long long)since(h, ac.last).launches, (unsigned long long)since(h, ac.last).epoch);
    if (h->cfg.max_episode_steps == 0)
        return fail(h, GYMNET_ERR_INVALID_ARG, "this handle has no time limit (max_episode_steps == 0): no episode is truncated and no row needs a boot");
    const void *obs = h->d_obs;
    int64_t obs_stride = h->ostride;
    if (h->autoreset) {
        // the terminal observation is gone from d_obs: the dense FINAL_OBS rows hold it, where they are maintained (make_step_args)
        if (!h->d_final_obs)
            return fail(h, GYMNET_ERR_INVALID_ARG, "on an auto-reset handle the terminal observation is read from the dense final-observation rows: "
                        "needs GYMNET_FLAG_FINAL_OBS");
        if (h->compact_only && h->d_done_list)
            return fail(h, GYMNET_ERR_INVALID_ARG, "GYMNET_FLAG_COMPACT_RECORDS_ONLY with GYMNET_FLAG_DONE_LIST does not maintain the dense final-observation "
                        "rows the boot reads");
        obs = h->d_final_obs;
        obs_stride = h->n;
    }
    if (ac.hist.n <= 0) return GYMNET_OK;
    HIP_TRY(h, h->f64 ? launch_boot_typed<double>(ac.critic, ac.hist, static_cast<const double *>(obs), obs_stride, h->d_done, d_boot, h->stream)
                      : launch_boot_typed<float>(ac.critic, ac.hist, static_cast<const float *>(obs), obs_stride, h->d_done, d_boot, h->stream));
    return GYMNET_OK;
    });
}

}  // extern "C"
