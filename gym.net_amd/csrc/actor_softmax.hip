// actor_softmax.hip — the Discrete actor (actor.hip) under an exploration setting other than its default: a lane whose coin says explore
// draws its action from softmax(logits / temperature) instead of uniformly over the actions.  The contract is
// gymnet_vecenv_actor_set_exploration in include/gymnet_amd.h.  With x[0 .. A) the logits, A = action_n <= 8:
//   greedy   the first index of the largest logit, m its value (argmax_value, actor_net.hpp: argmax_logits of actor.hip)
//   coin     word B of the aux stream <= coin_threshold(epsilon), as everywhere
//   UNIFORM  an exploring lane takes __umulhi(word A, A), as under the default setting (the host entry points send UNIFORM to actor.hip's
//            kernels, so this branch serves a caller inside the library only)
//   SOFTMAX  an exploring lane takes the first k with u * S < c_k, where e_k = exp_neg((x[k] - m) * inv_tau) (exp_neg.hpp), c_k = c_{k-1} +
//            e_k in index order, S = c_{A-1} and u = u01_24(word A of the action stream); the greedy action if there is none (u * S rounded
//            up to S, S = 0, NaN or infinite logits).  Every operation is float32 and rounds on its own, so tests/_actor_softmax_twin.py
//            reproduces the action bit for bit.  A chosen action has e_k > 0 or is the greedy one.  Word B is not u: on an exploring lane
//            it is small by construction.
// explore and inv_tau are wave-uniform kernel arguments, not template parameters: the forward pass dominates both the time and the register
// budget, and the draw comes after it, when at most eight values per lane are live.  The logits stay in the x[kW] register array: every
// loop over them is unrolled to 8 with a j < action_n guard, never a runtime index.
//
// Fused rollout (actor_softmax_rollout_kernel): actor_rollout_kernel with the setting as a fifth argument — rollout_body, one lane per
// thread, behind a hook whose choose() is the act kernel's body and whose after() is the shared push.  Both kernels call explore_compose_one,
// so the fused rollout is bit-identical to steps x (act, step, push).  The composition with its uniform draw is this unit's own copy:
// actor.hip's kernels stay instruction for instruction what they were.
#include "actor_net.hpp"
#include "exp_neg.hpp"

namespace gymnet {

namespace {

// the draw from softmax(x / tau) for one lane: u in [0, 1)
__device__ __forceinline__ int32_t softmax_draw(const float (&x)[kW], int32_t action_n, int32_t greedy, float m, float inv_tau, float u) {
    float c[8];
    float run = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (j < action_n) {                                                  // wave-uniform
            const float d = x[j] - m;
            const float a = d * inv_tau;
            run = run + exp_neg(a);
        }
        c[j] = run;
    }
    const float thr = u * run;
    int32_t act = greedy;
#pragma unroll
    for (int j = 7; j >= 0; --j) {                                           // descending: the first k with thr < c_k wins
        if (j < action_n && thr < c[j]) act = j;
    }
    return act;
}

// compose_one (actor.hip) under a setting: word A is drawn only when some lane of the wave explores, and the softmax runs under the same branch
__device__ __forceinline__ int32_t explore_compose_one(const float (&x)[kW], int32_t action_n, const ActorExplore &ex, uint32_t explore_at_or_below,
                                                       uint64_t seed, uint64_t gl, uint64_t tick) {
    float m;
    const int32_t greedy = argmax_value(x, action_n, m);
    const bool explore = aux_word<true>(seed, gl, tick) <= explore_at_or_below;
    int32_t act = greedy;
    if (__ballot(explore)) {
        const uint32_t wa = action_word<true>(seed, gl, tick);
        int32_t drawn;
        if (ex.explore == GYMNET_ACTOR_EXPLORE_SOFTMAX) drawn = softmax_draw(x, action_n, greedy, m, ex.inv_tau, u01_24(wa));   // wave-uniform
        else drawn = (int32_t)__umulhi(wa, (uint32_t)action_n);
        act = explore ? drawn : greedy;
    }
    return act;
}

}  // namespace

template <int O>
__global__ __launch_bounds__(256) void actor_softmax_act_kernel(const ActorNet net, const ActorHist hs, int32_t *__restrict__ actions,
                                                                float *__restrict__ logits, const ActorAct aa, const ActorExplore ex) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hs.n) return;
    float x[kW];
    load_input<O>(hs, hs.slot, i, x);
    actor_forward(net, x);
    if (logits) {
        for (int j = 0; j < net.action_n; ++j) {                               // (action_n <= 8: the Discrete envs' spaces)
            float v = x[0];
#pragma unroll
            for (int q = 1; q < 8; ++q) v = q == j ? x[q] : v;
            logits[i * net.action_n + j] = v;
        }
    }
    actions[i] = explore_compose_one(x, net.action_n, ex, coin_threshold(aa.epsilon), aa.seed, aa.lane_offset + (uint64_t)i, aa.tick);
}

// ActorHook (actor.hip) with the setting
template <class Env>
struct ActorSoftmaxHook {
    static constexpr bool CHOOSES = true;
    static constexpr int S = Env::S, O = Env::O;
    static_assert(std::is_same<typename Env::Real, float>::value && !Env::BOX_ACTION, "the actor serves float32 Discrete envs, one lane per thread");
    const ActorNet &net;
    const ActorHist &hs;
    const RolloutArgs &ro;
    const ActorExplore &ex;
    uint32_t explore_at_or_below;
    uint64_t lane_offset;
    int32_t newest;

    // gymnet_vecenv_actor_act_device(epsilon, action_seed, action_tick0 + t) under the handle's setting
    __device__ __forceinline__ void choose(int64_t t, int64_t i, int32_t (&act)[1]) const {
        float x[kW];
        load_input<O>(hs, newest, i, x);
        actor_forward(net, x);
        act[0] = explore_compose_one(x, net.action_n, ex, explore_at_or_below, ro.action_seed, lane_offset + (uint64_t)i, ro.action_tick0 + (uint64_t)t);
    }

    // gymnet_vecenv_actor_push_device (actor_net.hpp)
    __device__ __forceinline__ void after(int64_t, int64_t i, const uint8_t (&done)[1], const float (&s)[S][1], const float (&o)[O][1]) {
        hook_push<Env>(hs, newest, i, done, s, o);
    }
};

// actor_rollout_kernel (actor.hip) with the setting as a fifth argument: the same prologue (written out, see there), reset-form choice and
// launch bounds policy, then rollout_body with the hook above
template <class Env, bool AUTORESET, bool EXTRAS, bool RECORDS>
__global__ __launch_bounds__(256, kActorMinBlocks<EXTRAS>) void actor_softmax_rollout_kernel(const StepArgs a, const RolloutArgs ro, const ActorNet net,
                                                                                            const ActorHist hs, const ActorExplore ex) {
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
    const ActorSoftmaxHook<Env> hook{net, hs, ro, ex, coin_threshold(ro.epsilon), a.lane_offset, hs.slot};
    rollout_body<Env, 1, AUTORESET, false, EXTRAS, false, RESETF ? 1 : 0, RECORDS ? 1 : 0>(a, ro, i, tick0, sc, stage, hook);
}

template <class Env>
static hipError_t launch_softmax_rollout_env(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r) {
    const auto k = pick_rollout_form(h->autoreset, h->extras, records, [](auto ar, auto ex, auto rec) { return actor_softmax_rollout_kernel<Env, ar, ex, rec>; });
    hipLaunchKernelGGL(k, lane_grid(a.n), dim3(256), 0, h->stream, a, r, h->actor->net, h->actor->hist, actor_explore(*h->actor));
    return hipGetLastError();
}

hipError_t actor_softmax_rollout_launch(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r) {
    switch (h->cfg.env_id) {
        case GYMNET_ENV_CARTPOLE: return launch_softmax_rollout_env<CartPole>(h, records, a, r);
        case GYMNET_ENV_MOUNTAINCAR: return launch_softmax_rollout_env<MountainCar>(h, records, a, r);
        case GYMNET_ENV_ACROBOT: return launch_softmax_rollout_env<Acrobot>(h, records, a, r);
        default: return hipErrorInvalidValue;
    }
}

hipError_t actor_softmax_act_launch(const ActorNet &net, const ActorHist &hs, int32_t *actions, float *logits, const ActorAct &aa,
                                    const ActorExplore &ex, hipStream_t st) {
    if (hs.n <= 0) return hipSuccess;
    switch (hs.obs_dim) {
        case 2: hipLaunchKernelGGL(actor_softmax_act_kernel<2>, lane_grid(hs.n), dim3(256), 0, st, net, hs, actions, logits, aa, ex); break;
        case 4: hipLaunchKernelGGL(actor_softmax_act_kernel<4>, lane_grid(hs.n), dim3(256), 0, st, net, hs, actions, logits, aa, ex); break;
        case 6: hipLaunchKernelGGL(actor_softmax_act_kernel<6>, lane_grid(hs.n), dim3(256), 0, st, net, hs, actions, logits, aa, ex); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace gymnet

using namespace gymnet;

extern "C" {

int gymnet_vecenv_actor_set_exploration(gymnet_vecenv *h, int32_t explore, float temperature) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_actor(h));
    if (h->actor->box) return fail(h, GYMNET_ERR_INVALID_ARG, "this handle's actor chooses Box actions: an exploration setting belongs to a Discrete actor");
    if (explore != GYMNET_ACTOR_EXPLORE_UNIFORM && explore != GYMNET_ACTOR_EXPLORE_SOFTMAX) return fail(h, GYMNET_ERR_INVALID_ARG, "unknown explore %d", explore);
    const float inv_tau = 1.0f / temperature;
    if (!(__builtin_isfinite(temperature) && temperature > 0.0f && __builtin_isfinite(inv_tau)))
        return fail(h, GYMNET_ERR_INVALID_ARG, "temperature must be finite, > 0 and large enough for a finite 1 / temperature");
    Actor &ac = *h->actor;
    ac.discrete_explore = explore; ac.temperature = temperature; ac.inv_tau = inv_tau;   // read at the next act / actor rollout launch: ordered on the stream
    return GYMNET_OK;
    });
}

int gymnet_vecenv_actor_get_exploration(gymnet_vecenv *h, int32_t *explore, float *temperature) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_actor(h));
    if (h->actor->box) return fail(h, GYMNET_ERR_INVALID_ARG, "this handle's actor chooses Box actions: an exploration setting belongs to a Discrete actor");
    const Actor &ac = *h->actor;
    if (explore) *explore = ac.discrete_explore;
    if (temperature) *temperature = ac.temperature;
    return GYMNET_OK;
    });
}

}  // extern "C"
