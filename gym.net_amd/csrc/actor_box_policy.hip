// actor_box_policy.hip — the Box actor (actor_box.hip) under a policy other than its default: a tanh head and Gaussian exploration noise
// around the policy's action.  The contract is gymnet_vecenv_actor_box_set_policy in include/gymnet_amd.h.  With raw the network's one
// output and (low, high) the env's bounds:
//   greedy   CLAMP: raw < low ? low : (raw > high ? high : raw)   TANH: mid + half * tanh(raw), mid = (low + high) / 2, half = (high - low) / 2,
//            the product and the sum rounded on their own; a NaN passes either
//   coin     word B of the aux stream <= coin_threshold(epsilon), as everywhere
//   SAMPLE   an exploring lane takes low + (high - low) * u01_24(word A), as under the default policy
//   GAUSSIAN an exploring lane takes clamp(greedy + sigma * z), z = sqrt(-2 ln u1) * cos(2 pi u2): u1 = ((A >> 8) + 1) * 2^-24 from word A
//            of the action stream (the u1 of the Box sampler's unbounded regime, kernels.hip), u2 = u01_24(word N of the noise stream,
//            philox.hpp).  The cosine is the envs' own sincos_f32<true>: the angle lies in [0, 2 pi), so the library's large-argument path
//            would be dead weight in 14 kernels.
// head and explore are wave-uniform kernel arguments, not template parameters: the forward pass dominates both the time and the register
// budget, and the policy's few branches come after it, when one value per lane is live.
//
// Fused rollout (actor_box_policy_rollout_kernel): actor_box_rollout_kernel with the policy as a fifth argument — rollout_body, one lane
// per thread, behind a hook whose choose() is the act kernel's body and whose after() is the shared push.  Both kernels call policy_choose,
// (actor_box_compose.hpp, which actor_box_logd.hip runs too), so the fused rollout is bit-identical to steps x (box_act, step, push)
// whichever tanh / log / cos that function uses.
#include "actor_box_compose.hpp"

namespace gymnet {

template <int O>
__global__ __launch_bounds__(256) void actor_box_policy_act_kernel(const ActorNet net, const ActorHist hs, float *__restrict__ actions,
                                                                   float *__restrict__ raw, float low, float high, const ActorAct aa, const BoxPolicy pol) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hs.n) return;
    float r, g;
    actions[i] = policy_choose<O>(net, hs, hs.slot, i, low, high, pol, coin_threshold(aa.epsilon), aa.seed, aa.lane_offset + (uint64_t)i, aa.tick, r, g);
    if (raw) raw[i] = r;
}

// ActorBoxHook (actor_box.hip) with the policy
template <class Env>
struct ActorBoxPolicyHook {
    static constexpr bool CHOOSES = true;
    static constexpr int S = Env::S, O = Env::O;
    static_assert(std::is_same<typename Env::Real, float>::value && Env::BOX_ACTION, "the Box actor serves float32 Box envs, one lane per thread");
    const ActorNet &net;
    const ActorHist &hs;
    const RolloutArgs &ro;
    const BoxPolicy &pol;
    uint32_t explore_at_or_below;
    uint64_t lane_offset;
    int32_t newest;

    // gymnet_vecenv_actor_box_act_device(epsilon, action_seed, action_tick0 + t) under the handle's policy
    __device__ __forceinline__ void choose(int64_t t, int64_t i, float (&act)[1]) const {
        float raw, g;
        act[0] = policy_choose<O>(net, hs, newest, i, Env::ACTION_LOW, Env::ACTION_HIGH, pol, explore_at_or_below, ro.action_seed, lane_offset + (uint64_t)i,
                                  ro.action_tick0 + (uint64_t)t, raw, g);
    }

    // gymnet_vecenv_actor_push_device (actor_net.hpp)
    __device__ __forceinline__ void after(int64_t, int64_t i, const uint8_t (&done)[1], const float (&s)[S][1], const float (&o)[O][1]) {
        hook_push<Env>(hs, newest, i, done, s, o);
    }
};

// actor_box_rollout_kernel (actor_box.hip) with the policy as a fifth argument: the same prologue (written out, see actor.hip), reset-form
// choice and launch bounds policy, then rollout_body with the hook above
template <class Env, bool AUTORESET, bool EXTRAS, bool RECORDS>
__global__ __launch_bounds__(256, kActorMinBlocks<EXTRAS>) void actor_box_policy_rollout_kernel(const StepArgs a, const RolloutArgs ro, const ActorNet net,
                                                                                               const ActorHist hs, const BoxPolicy pol) {
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
    const ActorBoxPolicyHook<Env> hook{net, hs, ro, pol, coin_threshold(ro.epsilon), a.lane_offset, hs.slot};
    rollout_body<Env, 1, AUTORESET, false, EXTRAS, false, RESETF ? 1 : 0, RECORDS ? 1 : 0>(a, ro, i, tick0, sc, stage, hook);
}

template <class Env>
static hipError_t launch_policy_rollout_env(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r) {
    const auto k = pick_rollout_form(h->autoreset, h->extras, records, [](auto ar, auto ex, auto rec) { return actor_box_policy_rollout_kernel<Env, ar, ex, rec>; });
    hipLaunchKernelGGL(k, lane_grid(a.n), dim3(256), 0, h->stream, a, r, h->actor->net, h->actor->hist, box_policy(*h->actor));
    return hipGetLastError();
}

hipError_t actor_box_policy_rollout_launch(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r) {
    switch (h->cfg.env_id) {
        case GYMNET_ENV_PENDULUM: return launch_policy_rollout_env<Pendulum>(h, records, a, r);
        case GYMNET_ENV_MOUNTAINCAR_CONTINUOUS: return launch_policy_rollout_env<MountainCarContinuous>(h, records, a, r);
        default: return hipErrorInvalidValue;
    }
}

hipError_t actor_box_policy_act_launch(const ActorNet &net, const ActorHist &hs, float *actions, float *raw, float low, float high, const ActorAct &aa,
                                       const BoxPolicy &pol, hipStream_t st) {
    if (hs.n <= 0) return hipSuccess;
    switch (hs.obs_dim) {
        case 2: hipLaunchKernelGGL(actor_box_policy_act_kernel<2>, lane_grid(hs.n), dim3(256), 0, st, net, hs, actions, raw, low, high, aa, pol); break;
        case 3: hipLaunchKernelGGL(actor_box_policy_act_kernel<3>, lane_grid(hs.n), dim3(256), 0, st, net, hs, actions, raw, low, high, aa, pol); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace gymnet

using namespace gymnet;

extern "C" {

int gymnet_vecenv_actor_box_set_policy(gymnet_vecenv *h, int32_t head, int32_t explore, float sigma) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_actor(h));
    if (!h->actor->box) return fail(h, GYMNET_ERR_INVALID_ARG, "this handle's actor chooses Discrete actions: a policy belongs to a Box actor");
    if (head != GYMNET_BOX_HEAD_CLAMP && head != GYMNET_BOX_HEAD_TANH) return fail(h, GYMNET_ERR_INVALID_ARG, "unknown head %d", head);
    if (explore != GYMNET_BOX_EXPLORE_SAMPLE && explore != GYMNET_BOX_EXPLORE_GAUSSIAN) return fail(h, GYMNET_ERR_INVALID_ARG, "unknown explore %d", explore);
    if (!(__builtin_isfinite(sigma) && sigma >= 0.0f)) return fail(h, GYMNET_ERR_INVALID_ARG, "sigma must be finite and >= 0");
    Actor &ac = *h->actor;
    ac.head = head; ac.explore = explore; ac.sigma = sigma;                  // read at the next act / actor rollout launch: ordered on the stream
    return GYMNET_OK;
    });
}

int gymnet_vecenv_actor_box_get_policy(gymnet_vecenv *h, int32_t *head, int32_t *explore, float *sigma) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_actor(h));
    if (!h->actor->box) return fail(h, GYMNET_ERR_INVALID_ARG, "this handle's actor chooses Discrete actions: a policy belongs to a Box actor");
    const Actor &ac = *h->actor;
    if (head) *head = ac.head;
    if (explore) *explore = ac.explore;
    if (sigma) *sigma = ac.sigma;
    return GYMNET_OK;
    });
}

}  // extern "C"
