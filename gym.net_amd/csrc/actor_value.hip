// actor_value.hip — the critic: a second fully connected ReLU network attached to a configured actor, whose one output is the lane's
// value estimate.  The contract is gymnet_vecenv_actor_critic_config and its siblings in include/gymnet_amd.h.  The critic uses the
// actor's packed layout and limits (at most 4 layers, widths <= 64, <= 8192 parameters); its first width is the actor's input width,
// history * obs_dim, its last width 1; depth and hidden widths are its own.  Its value for a lane is actor_forward (actor_net.hpp) of
// the critic's weights over the input load_input gives for that lane, output 0: the same exact fmaf chain in the same order that gives
// the actor its logits.  No new arithmetic is specified: tests/_actor_twin.py's forward reproduces the value bit for bit up to the
// sign of a zero (twin.same).
//
// Stand-alone (actor_value_kernel): one lane per thread, weights through the scalar-cache view, templated on obs_dim like the act
// kernels; it serves every handle an actor serves, Box actors and float64 CartPole handles included (the history is float32 there too).
//
// Fused rollout (actor_value_rollout_kernel): actor_logp_rollout_kernel with the critic's network and the value pointer as further
// arguments — the written-out prologue, rollout_body, one lane per thread, behind a hook whose choose() composes the action with
// compose_one_logp (actor_compose_logp.hpp, the function actor_logp.hip runs: actions and logp are the same bits under both exploration
// settings), stores logp where the pointer is not null (a wave-uniform branch: one kernel per form), then loads the input AGAIN, runs
// the critic over it and stores output 0 at rec_value + t * n + i.  Loading twice keeps one x[64] live at a time; holding the input
// across the first network would double it.  after() is the shared push: bit-identical to steps x (act_value, step, push).
//
// A Box actor's values inside the fused rollout are actor_box_logd.hip's; V(terminal observation) for gymnet_gae_device's boot rows is
// actor_boot.hip's, for both kinds.  Out of scope: a trunk shared between actor and critic, values carried through the episode memory,
// and any gradient.
#include "actor_compose_logp.hpp"

namespace gymnet {

template <int O>
__global__ __launch_bounds__(256) void actor_value_kernel(const ActorNet critic, const ActorHist hs, float *__restrict__ value) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hs.n) return;
    float x[kW];
    load_input<O>(hs, hs.slot, i, x);
    actor_forward(critic, x);
    value[i] = x[0];
}

// ActorLogpHook (actor_logp.hip) that also records the critic's value of the input the action was chosen from.  Both record rows are
// pinned to SGPRs (lanes.hpp wave_uniform, that hook's SCALAR_ROW) in every form: against one 64-bit vector address each it allocates
// 0-4 VGPRs fewer in all 18 forms and leaves scratch in two forms instead of three (profiles/kernel_resources_actor_value.txt)
template <class Env>
struct ActorValueHook {
    static constexpr bool CHOOSES = true;
    static constexpr int S = Env::S, O = Env::O;
    static_assert(std::is_same<typename Env::Real, float>::value && !Env::BOX_ACTION, "the actor serves float32 Discrete envs, one lane per thread");
    const ActorNet &net;
    const ActorNet &critic;
    const ActorHist &hs;
    const RolloutArgs &ro;
    const ActorExplore &ex;
    float *__restrict__ rec_logp;                                            // [steps][n], or null
    float *__restrict__ rec_value;                                           // [steps][n]
    int64_t n;
    uint32_t explore_at_or_below;
    uint64_t lane_offset;
    int32_t newest;

    // gymnet_vecenv_actor_act_value_device(epsilon, action_seed, action_tick0 + t) under the handle's setting
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

    // gymnet_vecenv_actor_push_device (actor_net.hpp)
    __device__ __forceinline__ void after(int64_t, int64_t i, const uint8_t (&done)[1], const float (&s)[S][1], const float (&o)[O][1]) {
        hook_push<Env>(hs, newest, i, done, s, o);
    }
};

// actor_logp_rollout_kernel (actor_logp.hip) with the critic and the value pointer: the same prologue (written out, see actor.hip),
// reset-form choice and launch bounds policy, then rollout_body with the hook above
template <class Env, bool AUTORESET, bool EXTRAS, bool RECORDS>
__global__ __launch_bounds__(256, kActorMinBlocks<EXTRAS>) void actor_value_rollout_kernel(const StepArgs a, const RolloutArgs ro, const ActorNet net,
                                                                                          const ActorHist hs, const ActorExplore ex, const ActorNet critic,
                                                                                          float *__restrict__ rec_logp, float *__restrict__ rec_value) {
    constexpr bool RESETF = Env::OBS_ALIASES_STATE && AUTORESET;         // the wave-compacted reset where the env has it
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
        if (blockIdx.x == 0 && a.done_count2)
            for (int sh = threadIdx.x; sh < kShards; sh += blockDim.x) a.done_count2[(a.cparity ^ 1) * (kShards * kCountStride) + sh * kCountStride] = 0u;
    }
    // every lane of the thread is in range past this line (no GUARD form), and the active lanes of the last wave are a prefix (the
    // wave-level helpers rely on it)
    if (i >= a.n) return;
    const ActorValueHook<Env> hook{net, critic, hs, ro, ex, rec_logp, rec_value, a.n, coin_threshold(ro.epsilon), a.lane_offset, hs.slot};
    rollout_body<Env, 1, AUTORESET, false, EXTRAS, false, RESETF ? 1 : 0, RECORDS ? 1 : 0>(a, ro, i, tick0, sc, stage, hook);
}

template <class Env>
static hipError_t launch_value_rollout_env(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r, float *rec_logp, float *rec_value) {
    const auto k = pick_rollout_form(h->autoreset, h->extras, records, [](auto ar, auto ex, auto rec) { return actor_value_rollout_kernel<Env, ar, ex, rec>; });
    const Actor &ac = *h->actor;
    hipLaunchKernelGGL(k, lane_grid(a.n), dim3(256), 0, h->stream, a, r, ac.net, ac.hist, actor_explore(ac), ac.critic, rec_logp, rec_value);
    return hipGetLastError();
}

// actor.hip's router sends a Discrete actor's rollout with a value pointer here, under either setting, with or without a logp pointer
hipError_t actor_value_rollout_launch(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r, float *rec_logp, float *rec_value) {
    if (!h->actor->has_critic()) return hipErrorInvalidValue;               // (the plan has refused it: rollout_plan.hpp)
    switch (h->cfg.env_id) {
        case GYMNET_ENV_CARTPOLE: return launch_value_rollout_env<CartPole>(h, records, a, r, rec_logp, rec_value);
        case GYMNET_ENV_MOUNTAINCAR: return launch_value_rollout_env<MountainCar>(h, records, a, r, rec_logp, rec_value);
        case GYMNET_ENV_ACROBOT: return launch_value_rollout_env<Acrobot>(h, records, a, r, rec_logp, rec_value);
        default: return hipErrorInvalidValue;
    }
}

namespace {

hipError_t launch_value(const ActorNet &critic, const ActorHist &hs, float *value, hipStream_t st) {
    if (hs.n <= 0) return hipSuccess;
    switch (hs.obs_dim) {
        case 2: hipLaunchKernelGGL(actor_value_kernel<2>, lane_grid(hs.n), dim3(256), 0, st, critic, hs, value); break;
        case 3: hipLaunchKernelGGL(actor_value_kernel<3>, lane_grid(hs.n), dim3(256), 0, st, critic, hs, value); break;
        case 4: hipLaunchKernelGGL(actor_value_kernel<4>, lane_grid(hs.n), dim3(256), 0, st, critic, hs, value); break;
        case 6: hipLaunchKernelGGL(actor_value_kernel<6>, lane_grid(hs.n), dim3(256), 0, st, critic, hs, value); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// what a value costs to ask for, behind ENTER and need_actor: a critic, a pointer, a current history
int value_enter(gymnet_vecenv *h, const float *d_value) {
    if (!h->actor->has_critic()) return fail(h, GYMNET_ERR_INVALID_ARG, "no critic configured (gymnet_vecenv_actor_critic_config)");
    if (!d_value) return fail(h, GYMNET_ERR_INVALID_ARG, "d_value is null");
    if (!aligned_to(d_value, 4)) return fail(h, GYMNET_ERR_INVALID_ARG, "d_value must be 4-byte aligned");
    if (!actor_current(h))
        return fail(h, GYMNET_ERR_INVALID_ARG, "the actor's history is stale: push after every single vector step (or reset the actor; after a reset, "
                    "seed, set_tick or set_state of the handle only a reset of the actor serves)");
    return GYMNET_OK;
}

int critic_remove(gymnet_vecenv *h) {
    Actor &ac = *h->actor;
    ST_TRY(ac.critic_mem.release(h));
    ac.critic = ActorNet{};
    ac.critic_count = ac.critic_packed = 0;
    return GYMNET_OK;
}

}  // namespace

}  // namespace gymnet

using namespace gymnet;

extern "C" {

int gymnet_vecenv_actor_critic_config(gymnet_vecenv *h, int32_t num_layers, const int32_t *widths, const float *weights, int64_t count) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_actor(h));
    if (num_layers == 0) return critic_remove(h);
    Actor &ac = *h->actor;
    if (num_layers < 1 || num_layers > kActorMaxLayers) return fail(h, GYMNET_ERR_INVALID_ARG, "num_layers %d not in [0, %d]", num_layers, kActorMaxLayers);
    if (!widths || !weights) return fail(h, GYMNET_ERR_INVALID_ARG, "widths / weights is null");
    int64_t params = 0;
    ST_TRY(actor_net_check(h, num_layers, widths, count, ac.hist.history * ac.hist.obs_dim, 1, "the critic's one value", params));
    ActorNet net{};
    const int64_t packed_count = actor_net_shape(net, num_layers, widths);
    // the packed block and the weights as given (the pack kernel's input): both, or the old critic stays
    DeviceAllocs fresh;
    const size_t flat_bytes = sizeof(float) * (size_t)params;
    float *packed = static_cast<float *>(fresh.take(sizeof(float) * (size_t)packed_count));
    float *flat = packed ? static_cast<float *>(fresh.take(flat_bytes)) : nullptr;
    if (!flat) return fail(h, GYMNET_ERR_OOM, "hipMalloc of the critic (%lld parameters) failed", (long long)params);
    net.w = packed;
    ST_TRY(critic_remove(h));
    ac.critic_mem.ptrs.swap(fresh.ptrs);
    ac.critic = net; ac.critic_count = params; ac.critic_packed = packed_count;
    HIP_TRY(h, hipMemcpyAsync(flat, weights, flat_bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, launch_actor_pack(net, flat, packed, packed_count, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));     // the caller's host weights may go away when we return
    return GYMNET_OK;
    });
}

int gymnet_vecenv_actor_critic_load_device(gymnet_vecenv *h, const float *d_weights, int64_t count) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_actor(h));
    const Actor &ac = *h->actor;
    if (!ac.has_critic()) return fail(h, GYMNET_ERR_INVALID_ARG, "no critic configured (gymnet_vecenv_actor_critic_config)");
    if (!d_weights) return fail(h, GYMNET_ERR_INVALID_ARG, "d_weights is null");
    if (count != ac.critic_count) return fail(h, GYMNET_ERR_INVALID_ARG, "count %lld != the critic's %lld parameters", (long long)count, (long long)ac.critic_count);
    HIP_TRY(h, launch_actor_pack(ac.critic, d_weights, const_cast<float *>(ac.critic.w), ac.critic_packed, h->stream));
    return GYMNET_OK;
    });
}

int gymnet_vecenv_actor_value_device(gymnet_vecenv *h, float *d_value) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_actor(h));
    ST_TRY(value_enter(h, d_value));
    HIP_TRY(h, launch_value(h->actor->critic, h->actor->hist, d_value, h->stream));
    return GYMNET_OK;
    });
}

int gymnet_vecenv_actor_act_value_device(gymnet_vecenv *h, int32_t *d_actions, float *d_logits, float *d_logp, float *d_value, float epsilon,
                                         uint64_t seed, uint64_t tick) {
    if (!d_value) return gymnet_vecenv_actor_act_logp_device(h, d_actions, d_logits, d_logp, epsilon, seed, tick);
    return guarded([&]() -> int {
    ENTER(h);
    ActorAct aa;
    ST_TRY(actor_act_enter(h, false, "this handle's actor chooses Box actions: gymnet_vecenv_actor_box_act_device, then gymnet_vecenv_actor_value_device",
                           d_actions, d_logp, epsilon, seed, tick, aa));
    ST_TRY(value_enter(h, d_value));
    // the act launch the call without d_value makes, then the value kernel behind it on the stream
    HIP_TRY(h, actor_act_launch(h, d_actions, d_logits, d_logp, aa));
    HIP_TRY(h, launch_value(h->actor->critic, h->actor->hist, d_value, h->stream));
    return GYMNET_OK;
    });
}

}  // extern "C"
