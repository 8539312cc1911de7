// actor_box.hip — the on-device actor on a Box action space (Pendulum, MountainCarContinuous): the network, history and forward pass of
// actor.hip (actor_net.hpp) with a continuous head.  The last layer is one wide; its value `raw`, clamped to the env's bounds in the
// form the envs use (a NaN passes), is the greedy action, and exploration is TrainingPlaySession.ComposeAction (TrainingPlaySession.cs:
// 46-52) carried over to a Box space: where word B of the aux stream is at or below coin_threshold(epsilon) the action is
// ActionSpace.Sample() = low + (high - low) * u01_24(word A of the action stream), the value gymnet_vecenv_sample_actions_device writes
// for the same (seed, global lane, tick).  The contract is gymnet_vecenv_actor_box_config in include/gymnet_amd.h.  That is the default
// policy; any other (gymnet_vecenv_actor_box_set_policy: tanh head, Gaussian noise) runs the kernels of actor_box_policy.hip — the fused
// rollout by actor.hip's router, act by actor_box_act_launch below — and this unit's kernels stay what they were.
//
// Fused rollout (actor_box_rollout_kernel): step_kernels.hpp's rollout_body, one lane per thread, with a hook whose choose() is the act
// kernel's body and whose after() is the shared push: bit-identical to steps x (box_act, step, push).  Pendulum's observation has three
// rows, so this unit also compiles the push of a three-row history.
#include "actor_net.hpp"

namespace gymnet {

namespace {

// the envs' own clamp (Pendulum::step): a NaN fails both compares and passes
__device__ __forceinline__ float clamp_action(float raw, float low, float high) { return raw < low ? low : (raw > high ? high : raw); }

// the Box counterpart of actor.hip's compose_one: word B of the aux stream is the coin, word A of the action stream the sample
// (sample_box_kernel's bounded regime, Box.cs:85); the action word is drawn only when some lane of the wave explores
__device__ __forceinline__ float compose_box_one(float greedy, float low, float high, uint32_t explore_at_or_below, uint64_t seed, uint64_t gl,
                                                 uint64_t tick) {
    const bool explore = aux_word<true>(seed, gl, tick) <= explore_at_or_below;
    float act = greedy;
    if (__ballot(explore)) {
        const float drawn = low + (high - low) * u01_24(action_word<true>(seed, gl, tick));
        act = explore ? drawn : greedy;
    }
    return act;
}

// history -> forward -> raw -> clamp -> compose, for lane i; raw receives the unclamped output
template <int O>
__device__ __forceinline__ float box_choose(const ActorNet &net, const ActorHist &hs, int32_t newest, int64_t i, float low, float high,
                                            uint32_t explore_at_or_below, uint64_t seed, uint64_t gl, uint64_t tick, float &raw) {
    float x[kW];
    load_input<O>(hs, newest, i, x);
    actor_forward(net, x);
    raw = x[0];
    return compose_box_one(clamp_action(raw, low, high), low, high, explore_at_or_below, seed, gl, tick);
}

}  // namespace

template <int O>
__global__ __launch_bounds__(256) void actor_box_act_kernel(const ActorNet net, const ActorHist hs, float *__restrict__ actions, float *__restrict__ raw,
                                                            float low, float high, const ActorAct aa) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hs.n) return;
    float r;
    actions[i] = box_choose<O>(net, hs, hs.slot, i, low, high, coin_threshold(aa.epsilon), aa.seed, aa.lane_offset + (uint64_t)i, aa.tick, r);
    if (raw) raw[i] = r;
}

// rollout_body's hook for one lane per thread of a float32 Box env: newest is the ring slot of the newest observation
template <class Env>
struct ActorBoxHook {
    static constexpr bool CHOOSES = true;
    static constexpr int S = Env::S, O = Env::O;
    static_assert(std::is_same<typename Env::Real, float>::value && Env::BOX_ACTION, "the Box actor serves float32 Box envs, one lane per thread");
    const ActorNet &net;
    const ActorHist &hs;
    const RolloutArgs &ro;
    uint32_t explore_at_or_below;
    uint64_t lane_offset;
    int32_t newest;

    // gymnet_vecenv_actor_box_act_device(epsilon, action_seed, action_tick0 + t)
    __device__ __forceinline__ void choose(int64_t t, int64_t i, float (&act)[1]) const {
        float raw;
        act[0] = box_choose<O>(net, hs, newest, i, Env::ACTION_LOW, Env::ACTION_HIGH, explore_at_or_below, ro.action_seed, lane_offset + (uint64_t)i,
                               ro.action_tick0 + (uint64_t)t, raw);
    }

    // gymnet_vecenv_actor_push_device (actor_net.hpp)
    __device__ __forceinline__ void after(int64_t, int64_t i, const uint8_t (&done)[1], const float (&s)[S][1], const float (&o)[O][1]) {
        hook_push<Env>(hs, newest, i, done, s, o);
    }
};

// actor_rollout_kernel (actor.hip) for the Box envs: the same prologue (written out, see there) and launch bounds policy, then
// rollout_body with the hook above
template <class Env, bool AUTORESET, bool EXTRAS, bool RECORDS>
__global__ __launch_bounds__(256, kActorMinBlocks<EXTRAS>) void actor_box_rollout_kernel(const StepArgs a, const RolloutArgs ro, const ActorNet net, const ActorHist hs) {
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
            // Not vectorised, unlike actor.hip's copy: the two-wide form of this loop leaves a 32-byte stack temporary behind in the
            // MountainCarContinuous auto-reset bookkeeping form.  No instruction touches it, but the kernel would be launched with
            // scratch enabled.  This depends on the compiler; tests/test_actor_box_host.py's scratch == 0 assertion is what guards it.
#pragma clang loop vectorize(disable) interleave(disable)
            for (int sh = threadIdx.x; sh < kShards; sh += blockDim.x) a.done_count2[(a.cparity ^ 1) * (kShards * kCountStride) + sh * kCountStride] = 0u;
        }
    }
    // every lane of the thread is in range past this line (no GUARD form), and the active lanes of the last wave are a prefix (the
    // wave-level helpers rely on it)
    if (i >= a.n) return;
    const ActorBoxHook<Env> hook{net, hs, ro, coin_threshold(ro.epsilon), a.lane_offset, hs.slot};
    rollout_body<Env, 1, AUTORESET, false, EXTRAS, false, RESETF ? 1 : 0, RECORDS ? 1 : 0>(a, ro, i, tick0, sc, stage, hook);
}

template <class Env>
static hipError_t launch_actor_box_rollout_env(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r) {
    const auto k = pick_rollout_form(h->autoreset, h->extras, records, [](auto ar, auto ex, auto rec) { return actor_box_rollout_kernel<Env, ar, ex, rec>; });
    hipLaunchKernelGGL(k, lane_grid(a.n), dim3(256), 0, h->stream, a, r, h->actor->net, h->actor->hist);
    return hipGetLastError();
}

hipError_t actor_box_rollout_launch(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r) {
    switch (h->cfg.env_id) {
        case GYMNET_ENV_PENDULUM: return launch_actor_box_rollout_env<Pendulum>(h, records, a, r);
        case GYMNET_ENV_MOUNTAINCAR_CONTINUOUS: return launch_actor_box_rollout_env<MountainCarContinuous>(h, records, a, r);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_actor_box_push3(const ActorHist &hs, const float *obs, int64_t obs_stride, const uint8_t *restart, bool push, hipStream_t st) {
    hipLaunchKernelGGL((actor_push_kernel<float, 3>), lane_grid(hs.n), dim3(256), 0, st, hs, obs, obs_stride, restart, (int32_t)push);
    return hipGetLastError();
}

namespace {

hipError_t launch_actor_box_act(const ActorNet &net, const ActorHist &hs, float *actions, float *raw, float low, float high, const ActorAct &aa,
                                hipStream_t st) {
    if (hs.n <= 0) return hipSuccess;
    switch (hs.obs_dim) {
        case 2: hipLaunchKernelGGL(actor_box_act_kernel<2>, lane_grid(hs.n), dim3(256), 0, st, net, hs, actions, raw, low, high, aa); break;
        case 3: hipLaunchKernelGGL(actor_box_act_kernel<3>, lane_grid(hs.n), dim3(256), 0, st, net, hs, actions, raw, low, high, aa); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// which unit's act kernel serves the handle: the policy decides
hipError_t actor_box_act_launch(gymnet_vecenv *h, float *actions, float *raw, const ActorAct &aa) {
    const Actor &ac = *h->actor;
    const float low = h->desc->action_low, high = h->desc->action_high;
    if (!ac.default_policy()) return actor_box_policy_act_launch(ac.net, ac.hist, actions, raw, low, high, aa, box_policy(ac), h->stream);
    return launch_actor_box_act(ac.net, ac.hist, actions, raw, low, high, aa, h->stream);
}

}  // namespace

}  // namespace gymnet

using namespace gymnet;

extern "C" {

int gymnet_vecenv_actor_box_config(gymnet_vecenv *h, int32_t history, int32_t num_layers, const int32_t *widths, const float *weights,
                                   int64_t count) {
    return guarded([&]() -> int {
    ENTER(h);
    return actor_configure(h, true, history, num_layers, widths, weights, count);
    });
}

int gymnet_vecenv_actor_box_act_device(gymnet_vecenv *h, float *d_actions, float *d_raw, float epsilon, uint64_t seed, uint64_t tick) {
    return guarded([&]() -> int {
    ENTER(h);
    ActorAct aa;
    ST_TRY(actor_act_enter(h, true, "this handle's actor chooses Discrete actions: gymnet_vecenv_actor_act_device", d_actions, nullptr, epsilon, seed, tick, aa));
    HIP_TRY(h, actor_box_act_launch(h, d_actions, d_raw, aa));
    return GYMNET_OK;
    });
}

}  // extern "C"
