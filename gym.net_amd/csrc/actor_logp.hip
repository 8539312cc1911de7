// actor_logp.hip — the Discrete actor (actor.hip, actor_softmax.hip) when the caller also asks for the log-probability of the action each
// lane takes.  The contract is gymnet_vecenv_actor_act_logp_device in include/gymnet_amd.h.  With x[0 .. A) the logits, A = action_n <= 8,
// inv_tau the actor's stored 1 / temperature (whatever explore is) and j the action the lane takes, however it was chosen:
//   m      the greedy logit (argmax_value: step 1 of the softmax draw)
//   a_k    (x[k] - m) * inv_tau,  e_k = exp_neg(a_k),  S = (((e_0 + e_1) + ...) + e_{A-1}) in index order: steps 3-4 of the draw, computed
//          once per lane and shared with the draw where the wave draws
//   logp   a_j - log_pos(S) (log_pos.hpp), one subtraction; the canonical quiet NaN 0x7FC00000 if !(S >= 1) (an infinite or NaN greedy
//          logit: every weight is +0) or if the subtraction gives a NaN (uniform exploration took an action whose logit is NaN)
// a_j is selected by a compare-select chain over the unrolled register array, never a runtime index.  Every operation is float32 and
// rounds on its own, so tests/_actor_logp_twin.py reproduces the bits.  explore and inv_tau are wave-uniform kernel arguments as in
// actor_softmax.hip: one kernel serves both settings, and a request for logp always runs this unit, also under the default setting.
//
// The action is composed exactly as explore_compose_one (actor_softmax.hip) composes it — the same coin, the same words, the same c_k
// and threshold — so actions and logits are what act_device writes under the handle's setting.  The draw and the composition are a copy
// of actor_softmax.hip's (compose_one_logp in actor_compose_logp.hpp, which actor_value.hip includes too; argmax_value is
// actor_net.hpp's): the kernels of actor.hip and actor_softmax.hip stay instruction for instruction what they were.
//
// Fused rollout (actor_logp_rollout_kernel): actor_softmax_rollout_kernel with the record pointer as a sixth argument — rollout_body, one
// lane per thread, behind a hook whose choose() is the act kernel's body (it stores logp itself, at rec_logp + t * n + i) and whose
// after() is the shared push: bit-identical to steps x (act_logp, step, push).
#include "actor_compose_logp.hpp"

namespace gymnet {

template <int O>
__global__ __launch_bounds__(256) void actor_logp_act_kernel(const ActorNet net, const ActorHist hs, int32_t *__restrict__ actions,
                                                             float *__restrict__ logits, float *__restrict__ logp, const ActorAct aa,
                                                             const ActorExplore ex) {
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
    float lp;
    actions[i] = compose_one_logp(x, net.action_n, ex, coin_threshold(aa.epsilon), aa.seed, aa.lane_offset + (uint64_t)i, aa.tick, lp);
    logp[i] = lp;
}

// ActorSoftmaxHook (actor_softmax.hip) that records logp.  SCALAR_ROW: the step's row rec_logp + t * n is pinned to SGPRs (lanes.hpp
// wave_uniform) and the lane index added by the store, instead of one 64-bit vector address t * n + i.  The same bytes either way; the lean
// forms run at their launch bound of 168 VGPRs with over sixty SGPRs parked in VGPR lanes, and which form tips one address into scratch
// differs between them (docs/ledger.md §logp: measured per form, CartPole decides), so the kernel picks per form
template <class Env, bool SCALAR_ROW>
struct ActorLogpHook {
    static constexpr bool CHOOSES = true;
    static constexpr int S = Env::S, O = Env::O;
    static_assert(std::is_same<typename Env::Real, float>::value && !Env::BOX_ACTION, "the actor serves float32 Discrete envs, one lane per thread");
    const ActorNet &net;
    const ActorHist &hs;
    const RolloutArgs &ro;
    const ActorExplore &ex;
    float *__restrict__ rec_logp;                                            // [steps][n]
    int64_t n;
    uint32_t explore_at_or_below;
    uint64_t lane_offset;
    int32_t newest;

    // gymnet_vecenv_actor_act_logp_device(epsilon, action_seed, action_tick0 + t) under the handle's setting
    __device__ __forceinline__ void choose(int64_t t, int64_t i, int32_t (&act)[1]) const {
        float x[kW];
        load_input<O>(hs, newest, i, x);
        actor_forward(net, x);
        float lp;
        act[0] = compose_one_logp(x, net.action_n, ex, explore_at_or_below, ro.action_seed, lane_offset + (uint64_t)i, ro.action_tick0 + (uint64_t)t, lp);
        if constexpr (SCALAR_ROW) wave_uniform(rec_logp + t * n)[i] = lp;
        else rec_logp[t * n + i] = lp;
    }

    // gymnet_vecenv_actor_push_device (actor_net.hpp)
    __device__ __forceinline__ void after(int64_t, int64_t i, const uint8_t (&done)[1], const float (&s)[S][1], const float (&o)[O][1]) {
        hook_push<Env>(hs, newest, i, done, s, o);
    }
};

// actor_softmax_rollout_kernel (actor_softmax.hip) with the record pointer as a sixth argument: the same prologue (written out, see
// actor.hip), reset-form choice and launch bounds policy, then rollout_body with the hook above
template <class Env, bool AUTORESET, bool EXTRAS, bool RECORDS>
__global__ __launch_bounds__(256, kActorMinBlocks<EXTRAS>) void actor_logp_rollout_kernel(const StepArgs a, const RolloutArgs ro, const ActorNet net,
                                                                                         const ActorHist hs, const ActorExplore ex,
                                                                                         float *__restrict__ rec_logp) {
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
    const ActorLogpHook<Env, AUTORESET> hook{net, hs, ro, ex, rec_logp, a.n, coin_threshold(ro.epsilon), a.lane_offset, hs.slot};
    rollout_body<Env, 1, AUTORESET, false, EXTRAS, false, RESETF ? 1 : 0, RECORDS ? 1 : 0>(a, ro, i, tick0, sc, stage, hook);
}

template <class Env>
static hipError_t launch_logp_rollout_env(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r, float *rec_logp) {
    const auto k = pick_rollout_form(h->autoreset, h->extras, records, [](auto ar, auto ex, auto rec) { return actor_logp_rollout_kernel<Env, ar, ex, rec>; });
    hipLaunchKernelGGL(k, lane_grid(a.n), dim3(256), 0, h->stream, a, r, h->actor->net, h->actor->hist, actor_explore(*h->actor), rec_logp);
    return hipGetLastError();
}

// actor.hip's router sends a Discrete actor's rollout with a record pointer here, under either setting
hipError_t actor_logp_rollout_launch(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r, float *rec_logp) {
    switch (h->cfg.env_id) {
        case GYMNET_ENV_CARTPOLE: return launch_logp_rollout_env<CartPole>(h, records, a, r, rec_logp);
        case GYMNET_ENV_MOUNTAINCAR: return launch_logp_rollout_env<MountainCar>(h, records, a, r, rec_logp);
        case GYMNET_ENV_ACROBOT: return launch_logp_rollout_env<Acrobot>(h, records, a, r, rec_logp);
        default: return hipErrorInvalidValue;
    }
}

hipError_t actor_logp_act_launch(const ActorNet &net, const ActorHist &hs, int32_t *actions, float *logits, float *logp, const ActorAct &aa,
                                 const ActorExplore &ex, hipStream_t st) {
    if (hs.n <= 0) return hipSuccess;
    switch (hs.obs_dim) {
        case 2: hipLaunchKernelGGL(actor_logp_act_kernel<2>, lane_grid(hs.n), dim3(256), 0, st, net, hs, actions, logits, logp, aa, ex); break;
        case 4: hipLaunchKernelGGL(actor_logp_act_kernel<4>, lane_grid(hs.n), dim3(256), 0, st, net, hs, actions, logits, logp, aa, ex); break;
        case 6: hipLaunchKernelGGL(actor_logp_act_kernel<6>, lane_grid(hs.n), dim3(256), 0, st, net, hs, actions, logits, logp, aa, ex); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace gymnet

using namespace gymnet;

extern "C" {

int gymnet_vecenv_actor_act_logp_device(gymnet_vecenv *h, int32_t *d_actions, float *d_logits, float *d_logp, float epsilon, uint64_t seed,
                                        uint64_t tick) {
    if (!d_logp) return gymnet_vecenv_actor_act_device(h, d_actions, d_logits, epsilon, seed, tick);
    return guarded([&]() -> int {
    ENTER(h);
    ActorAct aa;
    ST_TRY(actor_act_enter(h, false, "this handle's actor chooses Box actions: a log-probability belongs to a Discrete actor", d_actions, d_logp, epsilon, seed, tick, aa));
    HIP_TRY(h, actor_act_launch(h, d_actions, d_logits, d_logp, aa));
    return GYMNET_OK;
    });
}

}  // extern "C"
