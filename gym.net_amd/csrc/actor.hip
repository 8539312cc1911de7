// actor.hip — the on-device actor: a small fully connected ReLU network, given by the caller, that chooses every lane's action from
// the lane's observation history (the trainer's BasePlaySession.ComposeAction -> Trainer.Predict -> _network.Forward, PlaySessions/
// BasePlaySession.cs:78-81, Trainer.cs:91-92, and TrainingPlaySession.cs:46-52's epsilon-greedy wrapper), in the single-step path and
// inside a fused rollout.  The contract is gymnet_vecenv_actor_config and its siblings in include/gymnet_amd.h; tests/_actor_twin.py
// restates it with an exact fmaf.  Written for gfx950 (wave64); compiled with -ffp-contract=off, so every multiply-add below is an
// explicit __builtin_fmaf.
//
// Forward (VALU form, docs/ledger.md §actor).  One env lane per thread.  The activations of a layer live in VGPRs (x[64], zero beyond the
// layer's width), the weights are wave-uniform and come through the scalar cache: the packed weight block (actor_pack_kernel) is read
// through an address-space-4 pointer, so each chunk of 4 neurons x 8 inputs is two s_load_dwordx16 and each multiply-add is one
// v_fma_f32 with an SGPR operand.  Neurons go four at a time (four independent fmaf chains per thread), inputs in chunks of eight; a
// wave-uniform branch skips the chunks and groups beyond the layer's real widths, and zero padding inside the last chunk / group only
// adds fmaf(0, 0, acc) terms after the real ones (exact, but for the sign of a zero sum).
//
// History.  float32 SoA [S][obs_dim][stride], a ring: every lane pushes together, so the newest observation goes to slot (slot + 1) % S
// for every lane and a push writes one observation per lane; a restarting lane (done byte set, or a masked reset) writes its
// observation into every slot.  Input row s (oldest first) of the network is ring slot (slot + 1 + s) % S.
//
// Fused rollout (actor_rollout_kernel).  step_kernels.hpp's rollout_body itself, one lane per thread, with a hook (ActorHook) that
// chooses the action of step t from the history and keeps that history current in memory: bit-identical to steps x (act, step, push).
// This unit instantiates its own kernels; the env_*.hip units are untouched.
//
// What the Box actor (actor_box.hip: Pendulum, MountainCarContinuous) shares with this unit — the network and history structs, the forward
// pass, load_input, the ring arithmetic, the push — is in actor_net.hpp; the Discrete head (argmax_logits, compose_one) stays here.
// That head is the default exploration setting; the other settings and policies have kernels of their own in the sibling units, and this
// unit's kernels stay what they were.
//
// The host side follows the kernels: gymnet_vecenv_actor_*, the handle's Actor attachment, the prologue of every act entry point
// (actor_act_enter), and the calls the fused rollout (rollout_fused.hip) makes when the actor chooses its actions.  actor_rollout_launch among them
// is the router: it alone says which of the eight units runs a handle's rollout (actor_act_launch: the same for act).
#include "actor_net.hpp"

namespace gymnet {

namespace {

// first index of the largest logit (moves only on a strictly greater value)
__device__ __forceinline__ int32_t argmax_logits(const float (&x)[kW], int32_t action_n) {
    int32_t best = 0;
    float bv = x[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) {
        if (j < action_n && x[j] > bv) { bv = x[j]; best = j; }
    }
    return best;
}

// gymnet_vecenv_compose_actions_device's choice for one lane: word B of the aux stream is the coin, word A of the action stream the
// sampled action (compose_discrete_kernel); the action word is drawn only when some lane of the wave explores
__device__ __forceinline__ int32_t compose_one(int32_t greedy, int32_t action_n, uint32_t explore_at_or_below, uint64_t seed, uint64_t gl,
                                               uint64_t tick) {
    const bool explore = aux_word<true>(seed, gl, tick) <= explore_at_or_below;
    int32_t act = greedy;
    if (__ballot(explore)) {
        const int32_t drawn = (int32_t)__umulhi(action_word<true>(seed, gl, tick), (uint32_t)action_n);
        act = explore ? drawn : greedy;
    }
    return act;
}

}  // namespace

template <int O>
__global__ __launch_bounds__(256) void actor_act_kernel(const ActorNet net, const ActorHist hs, int32_t *__restrict__ actions,
                                                        float *__restrict__ logits, const ActorAct aa) {
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
    const int32_t greedy = argmax_logits(x, net.action_n);
    actions[i] = compose_one(greedy, net.action_n, coin_threshold(aa.epsilon), aa.seed, aa.lane_offset + (uint64_t)i, aa.tick);
}

// gymnet_vecenv_actor_history_device: the ring unrolled, oldest first, into the caller's [history][obs_dim][out_stride]
__global__ __launch_bounds__(256) void actor_history_kernel(const ActorHist hs, float *__restrict__ out, int64_t out_stride) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hs.n) return;
    for (int32_t s = 0; s < hs.history; ++s) {
        const int32_t row = ring_row(hs.slot, s, hs.history);
        for (int32_t k = 0; k < hs.obs_dim; ++k)
            out[((int64_t)s * hs.obs_dim + k) * out_stride + i] = hs.hist[((int64_t)row * hs.obs_dim + k) * hs.stride + i];
    }
}

// flat torch layout (per layer W [wout][win] row-major, then b [wout]) -> the packed block actor_forward reads
__global__ __launch_bounds__(256) void actor_pack_kernel(const ActorNet net, const float *__restrict__ flat, float *__restrict__ packed,
                                                         int64_t packed_count) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= packed_count) return;
    int64_t fo = 0;
    float v = 0.0f;
    for (int l = 0; l < net.layers; ++l) {
        const int32_t win = net.win[l], wout = net.wout[l];
        const int64_t gf = group_floats(win);
        const int64_t end = net.off[l] + (int64_t)((wout + 3) >> 2) * gf;
        if (p >= net.off[l] && p < end) {
            const int64_t q = p - net.off[l];
            const int64_t g = q / gf, r = q % gf;
            if (r < 4) {
                const int64_t j = 4 * g + r;
                if (j < wout) v = flat[fo + (int64_t)wout * win + j];
            } else {
                const int64_t c = (r - 4) / 32, e = (r - 4) % 32;
                const int64_t j = 4 * g + e / 8, in = 8 * c + e % 8;
                if (j < wout && in < win) v = flat[fo + j * win + in];
            }
        }
        fo += (int64_t)wout * win + wout;
    }
    packed[p] = v;
}

// ---- the fused rollout with the actor choosing the actions -------------------------------------------------------------------------
// rollout_body's hook (step_kernels.hpp) for one lane per thread: the action of step t comes from the history, and the post-step
// observation goes back into it.  newest: the ring slot of the newest observation
template <class Env>
struct ActorHook {
    static constexpr bool CHOOSES = true;
    static constexpr int S = Env::S, O = Env::O;
    // choose() and after() are written for rollout_body<Env, 1, ...> of a float32 env with a Discrete action space
    static_assert(std::is_same<typename Env::Real, float>::value && !Env::BOX_ACTION, "the actor serves float32 Discrete envs, one lane per thread");
    const ActorNet &net;
    const ActorHist &hs;
    const RolloutArgs &ro;
    uint32_t explore_at_or_below;
    uint64_t lane_offset;
    int32_t newest;

    // gymnet_vecenv_actor_act_device(epsilon, action_seed, action_tick0 + t)
    __device__ __forceinline__ void choose(int64_t t, int64_t i, int32_t (&act)[1]) const {
        float x[kW];
        load_input<O>(hs, newest, i, x);
        actor_forward(net, x);
        act[0] = compose_one(argmax_logits(x, net.action_n), net.action_n, explore_at_or_below, ro.action_seed, lane_offset + (uint64_t)i, ro.action_tick0 + (uint64_t)t);
    }

    // gymnet_vecenv_actor_push_device (actor_net.hpp)
    __device__ __forceinline__ void after(int64_t, int64_t i, const uint8_t (&done)[1], const float (&s)[S][1], const float (&o)[O][1]) {
        hook_push<Env>(hs, newest, i, done, s, o);
    }
};

// rollout_kernel's prologue (step_kernels.hpp) with one lane per thread, then rollout_body with the hook above: bit-identical to
// steps x (act, step, push).  RECORDS: the rollout keeps compact episode records, with the overflow segment.  (The prologue is written
// out here and in actor_box_rollout_kernel: moved into a helper it changes the instruction streams of all 18 forms.)
template <class Env, bool AUTORESET, bool EXTRAS, bool RECORDS>
__global__ __launch_bounds__(256, kActorMinBlocks<EXTRAS>) void actor_rollout_kernel(const StepArgs a, const RolloutArgs ro, const ActorNet net, const ActorHist hs) {
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
    const ActorHook<Env> hook{net, hs, ro, coin_threshold(ro.epsilon), a.lane_offset, hs.slot};
    rollout_body<Env, 1, AUTORESET, false, EXTRAS, false, RESETF ? 1 : 0, RECORDS ? 1 : 0>(a, ro, i, tick0, sc, stage, hook);
}

template <class Env>
static hipError_t launch_actor_rollout_env(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r) {
    const auto k = pick_rollout_form(h->autoreset, h->extras, records, [](auto ar, auto ex, auto rec) { return actor_rollout_kernel<Env, ar, ex, rec>; });
    hipLaunchKernelGGL(k, lane_grid(a.n), dim3(256), 0, h->stream, a, r, h->actor->net, h->actor->hist);
    return hipGetLastError();
}

// the ActorNet of widths[0 .. layers] (w unset); returns the floats of its packed block, off[l] = where layer l starts
int64_t actor_net_shape(ActorNet &net, int32_t layers, const int32_t *widths) {
    net.layers = layers; net.action_n = widths[layers];
    int64_t total = 0;
    for (int l = 0; l < layers; ++l) {
        net.win[l] = widths[l]; net.wout[l] = widths[l + 1];
        net.off[l] = (int32_t)total;
        total += (int64_t)((widths[l + 1] + 3) >> 2) * group_floats(widths[l]);
    }
    return total;
}

hipError_t launch_actor_pack(const ActorNet &net, const float *flat, float *packed, int64_t packed_count, hipStream_t st) {
    hipLaunchKernelGGL(actor_pack_kernel, lane_grid(packed_count), dim3(256), 0, st, net, flat, packed, packed_count);
    return hipGetLastError();
}

namespace {

template <class R>
hipError_t launch_actor_push_typed(const ActorHist &hs, const R *obs, int64_t obs_stride, const uint8_t *restart, bool push, hipStream_t st) {
    switch (hs.obs_dim) {
        case 2: hipLaunchKernelGGL((actor_push_kernel<R, 2>), lane_grid(hs.n), dim3(256), 0, st, hs, obs, obs_stride, restart, (int32_t)push); break;
        case 3:                                       // Pendulum, float32 only: the kernel is actor_box.hip's
            if constexpr (sizeof(R) == 4) return launch_actor_box_push3(hs, obs, obs_stride, restart, push, st);
            else return hipErrorInvalidValue;
        case 4: hipLaunchKernelGGL((actor_push_kernel<R, 4>), lane_grid(hs.n), dim3(256), 0, st, hs, obs, obs_stride, restart, (int32_t)push); break;
        case 6: hipLaunchKernelGGL((actor_push_kernel<R, 6>), lane_grid(hs.n), dim3(256), 0, st, hs, obs, obs_stride, restart, (int32_t)push); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// push = true: lanes with restart[k] != 0 write every slot, the others slot hs.slot; push = false (reset): lanes with restart[k] != 0
// (NULL: every lane) write every slot, the others nothing.  obs: the CURRENT observation buffer, float or double (f64)
hipError_t launch_actor_push(bool f64, const ActorHist &hs, const void *obs, int64_t obs_stride, const uint8_t *restart, bool push,
                             hipStream_t st) {
    if (hs.n <= 0) return hipSuccess;
    if (f64) return launch_actor_push_typed<double>(hs, static_cast<const double *>(obs), obs_stride, restart, push, st);
    return launch_actor_push_typed<float>(hs, static_cast<const float *>(obs), obs_stride, restart, push, st);
}

hipError_t launch_actor_act(const ActorNet &net, const ActorHist &hs, int32_t *actions, float *logits, const ActorAct &aa, hipStream_t st) {
    if (hs.n <= 0) return hipSuccess;
    switch (hs.obs_dim) {
        case 2: hipLaunchKernelGGL(actor_act_kernel<2>, lane_grid(hs.n), dim3(256), 0, st, net, hs, actions, logits, aa); break;
        case 4: hipLaunchKernelGGL(actor_act_kernel<4>, lane_grid(hs.n), dim3(256), 0, st, net, hs, actions, logits, aa); break;
        case 6: hipLaunchKernelGGL(actor_act_kernel<6>, lane_grid(hs.n), dim3(256), 0, st, net, hs, actions, logits, aa); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

int release_actor(gymnet_vecenv *h) { return release_attachment(h, h->actor); }

namespace {

int actor_refill(gymnet_vecenv *h, const uint8_t *d_mask) {
    HIP_TRY(h, launch_actor_push(h->f64, h->actor->hist, h->d_obs, h->ostride, d_mask, false, h->stream));
    h->actor->last = mark(h);
    return GYMNET_OK;
}

}  // namespace

// what the fused rollout's plan (rollout_plan.hpp) reads of the handle's actor: its refusals are worded there
ActorFacts actor_facts(const gymnet_vecenv *h) {
    if (!h->actor) return {};
    return {h->actor->box ? ActorKind::Box : ActorKind::Discrete, h->actor->has_critic(), actor_current(h), h->actor->sigma};
}

// this unit's fused rollout: a Discrete actor under the default exploration setting
static hipError_t actor_discrete_rollout_launch(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r) {
    switch (h->cfg.env_id) {
        case GYMNET_ENV_CARTPOLE: return launch_actor_rollout_env<CartPole>(h, records, a, r);
        case GYMNET_ENV_MOUNTAINCAR: return launch_actor_rollout_env<MountainCar>(h, records, a, r);
        case GYMNET_ENV_ACROBOT: return launch_actor_rollout_env<Acrobot>(h, records, a, r);
        default: return hipErrorInvalidValue;
    }
}

// The router: which unit runs the fused rollout of this handle, as it stands at the launch.  Box: a log-density or value pointer
// (gymnet_vecenv_rollout_fused_box_logd_device) goes to actor_box_logd.hip under any policy, else its policy decides.  Discrete: a value
// pointer (gymnet_vecenv_rollout_fused_value_device) goes to actor_value.hip, with or without a logp pointer; a logp pointer alone
// (gymnet_vecenv_rollout_fused_logp_device) to actor_logp.hip under either setting; else the setting decides.  A boot pointer
// (gymnet_vecenv_rollout_fused_value_boot_device, _box_boot_device) goes to actor_boot.hip for either kind
hipError_t actor_rollout_launch(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r, const FusedRequest &rq) {
    const Actor &ac = *h->actor;
    if (a.n <= 0) return hipSuccess;
    if (rq.rec_boot)                                                         // (actor_boot.hip: both kinds)
        return ac.box ? actor_box_boot_rollout_launch(h, records, a, r, rq.rec_logd, rq.rec_value, rq.rec_boot)
                      : actor_value_boot_rollout_launch(h, records, a, r, rq.rec_logp, rq.rec_value, rq.rec_boot);
    if (ac.box) {
        if (rq.rec_logd || rq.box_value) return actor_box_logd_rollout_launch(h, records, a, r, rq.rec_logd, rq.box_value ? rq.rec_value : nullptr);
        if (rq.rec_logp || rq.rec_value) return hipErrorInvalidValue;        // (the plan has refused it: rollout_plan.hpp record_pointers)
        return ac.default_policy() ? actor_box_rollout_launch(h, records, a, r) : actor_box_policy_rollout_launch(h, records, a, r);
    }
    if (rq.rec_value) return actor_value_rollout_launch(h, records, a, r, rq.rec_logp, rq.rec_value);
    if (rq.rec_logp) return actor_logp_rollout_launch(h, records, a, r, rq.rec_logp);
    return ac.default_exploration() ? actor_discrete_rollout_launch(h, records, a, r) : actor_softmax_rollout_launch(h, records, a, r);
}

// the kernel pushed every step: the history is current, its newest slot moved `steps` on
void actor_rollout_done(gymnet_vecenv *h, int64_t steps) {
    ActorHist &hs = h->actor->hist;
    hs.slot = (int32_t)(((int64_t)hs.slot + steps) % hs.history);
    h->actor->last = mark(h);
}

// the router's counterpart for act on a Discrete handle: a logp pointer goes to actor_logp.hip under either setting, else the setting decides
hipError_t actor_act_launch(gymnet_vecenv *h, int32_t *actions, float *logits, float *logp, const ActorAct &aa) {
    const Actor &ac = *h->actor;
    if (logp) return actor_logp_act_launch(ac.net, ac.hist, actions, logits, logp, aa, actor_explore(ac), h->stream);
    if (!ac.default_exploration()) return actor_softmax_act_launch(ac.net, ac.hist, actions, logits, aa, actor_explore(ac), h->stream);
    return launch_actor_act(ac.net, ac.hist, actions, logits, aa, h->stream);
}

int actor_act_enter(gymnet_vecenv *h, bool want_box, const char *wrong_kind, const void *d_actions, const float *d_logp, float epsilon, uint64_t seed,
                    uint64_t tick, ActorAct &aa) {
    ST_TRY(need_actor(h));
    if (h->actor->box != want_box) return fail(h, GYMNET_ERR_INVALID_ARG, "%s", wrong_kind);
    if (!d_actions) return fail(h, GYMNET_ERR_INVALID_ARG, "d_actions is null");
    if (!aligned_to(d_logp, 4)) return fail(h, GYMNET_ERR_INVALID_ARG, "d_logp must be 4-byte aligned");
    if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return fail(h, GYMNET_ERR_INVALID_ARG, "epsilon must be in [0, 1]");
    if (!actor_current(h))
        return fail(h, GYMNET_ERR_INVALID_ARG, "the actor's history is stale: push after every single vector step (or reset the actor; after a reset, "
                    "seed, set_tick or set_state of the handle only a reset of the actor serves)");
    aa = ActorAct{epsilon, seed, (uint64_t)h->cfg.lane_offset, tick};
    return GYMNET_OK;
}

int actor_net_check(gymnet_vecenv *h, int32_t num_layers, const int32_t *widths, int64_t count, int32_t first, int32_t last, const char *last_name,
                    int64_t &params) {
    params = 0;
    for (int l = 0; l <= num_layers; ++l)
        if (widths[l] < 1 || widths[l] > kActorMaxWidth) return fail(h, GYMNET_ERR_INVALID_ARG, "width %d of layer boundary %d not in [1, %d]", widths[l], l, kActorMaxWidth);
    for (int l = 0; l < num_layers; ++l) params += (int64_t)widths[l + 1] * widths[l] + widths[l + 1];
    if (widths[0] != first) return fail(h, GYMNET_ERR_INVALID_ARG, "widths[0] %d != history * obs_dim = %d", widths[0], first);
    if (widths[num_layers] != last) return fail(h, GYMNET_ERR_INVALID_ARG, "widths[%d] %d != %s = %d", num_layers, widths[num_layers], last_name, last);
    if (params > kActorMaxParams) return fail(h, GYMNET_ERR_INVALID_ARG, "%lld parameters > %d", (long long)params, kActorMaxParams);
    if (count != params) return fail(h, GYMNET_ERR_INVALID_ARG, "count %lld != %lld parameters of these widths", (long long)count, (long long)params);
    return GYMNET_OK;
}

// gymnet_vecenv_actor_config (box = false) and gymnet_vecenv_actor_box_config (box = true) behind ENTER: the same network, history and
// checks; the kind must be the env's, and the last width is the Discrete space's n or the Box space's one dimension
int actor_configure(gymnet_vecenv *h, bool box, int32_t history, int32_t num_layers, const int32_t *widths, const float *weights, int64_t count) {
    if (num_layers == 0) return release_actor(h);
    const EnvDesc &d = *h->desc;
    if (d.box_action && !box)
        return fail(h, GYMNET_ERR_UNSUPPORTED, "the actor chooses Discrete actions; %s has a Box action space (gymnet_vecenv_actor_box_config)", d.name);
    if (!d.box_action && box)
        return fail(h, GYMNET_ERR_UNSUPPORTED, "the Box actor chooses Box actions; %s has a Discrete action space (gymnet_vecenv_actor_config)", d.name);
    if (box && h->f64) return fail(h, GYMNET_ERR_UNSUPPORTED, "the Box actor serves float32 handles");
    const int32_t last = box ? 1 : d.action_n;
    if (num_layers < 1 || num_layers > kActorMaxLayers) return fail(h, GYMNET_ERR_INVALID_ARG, "num_layers %d not in [0, %d]", num_layers, kActorMaxLayers);
    if (!widths || !weights) return fail(h, GYMNET_ERR_INVALID_ARG, "widths / weights is null");
    if (history < 1 || (int64_t)history * d.obs_dim > kActorMaxWidth)
        return fail(h, GYMNET_ERR_INVALID_ARG, "history %d: history * obs_dim must be in [1, %d]", history, kActorMaxWidth);
    if (!box && d.action_n > kActorMaxActions) return fail(h, GYMNET_ERR_UNSUPPORTED, "more than %d actions", kActorMaxActions);
    int64_t params = 0;
    ST_TRY(actor_net_check(h, num_layers, widths, count, history * d.obs_dim, last, box ? "the action dimension" : "action_n", params));
    std::unique_ptr<Actor> fresh(new Actor);
    fresh->box = box;
    ActorNet &net = fresh->net;
    fresh->count = params;
    fresh->packed = actor_net_shape(net, num_layers, widths);
    // the packed block, the weights as given (torch layout: the pack kernel's input) and the history: all three, or the old actor stays
    const size_t flat_bytes = sizeof(float) * (size_t)params;
    float *packed = static_cast<float *>(fresh->mem.take(sizeof(float) * (size_t)fresh->packed));
    float *flat = packed ? static_cast<float *>(fresh->mem.take(flat_bytes)) : nullptr;
    float *hist = flat ? static_cast<float *>(fresh->mem.take(sizeof(float) * (size_t)history * (size_t)d.obs_dim * (size_t)h->n)) : nullptr;
    if (!hist) return fail(h, GYMNET_ERR_OOM, "hipMalloc of the actor (%lld parameters, %d x %d x %lld history) failed", (long long)params, history, d.obs_dim, (long long)h->n);
    net.w = packed;
    ActorHist &hs = fresh->hist;
    hs.hist = hist; hs.stride = h->n; hs.history = history; hs.obs_dim = d.obs_dim; hs.slot = 0; hs.n = h->n;
    ST_TRY(release_actor(h));
    h->actor = fresh.release();
    HIP_TRY(h, hipMemcpyAsync(flat, weights, flat_bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, launch_actor_pack(net, flat, packed, h->actor->packed, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));     // the caller's host weights may go away when we return
    return actor_refill(h, nullptr);
}

}  // namespace gymnet

using namespace gymnet;

extern "C" {

int gymnet_vecenv_actor_config(gymnet_vecenv *h, int32_t history, int32_t num_layers, const int32_t *widths, const float *weights,
                               int64_t count) {
    return guarded([&]() -> int {
    ENTER(h);
    return actor_configure(h, false, history, num_layers, widths, weights, count);
    });
}

int gymnet_vecenv_actor_load_device(gymnet_vecenv *h, const float *d_weights, int64_t count) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_actor(h));
    const Actor &ac = *h->actor;
    if (!d_weights) return fail(h, GYMNET_ERR_INVALID_ARG, "d_weights is null");
    if (count != ac.count) return fail(h, GYMNET_ERR_INVALID_ARG, "count %lld != the actor's %lld parameters", (long long)count, (long long)ac.count);
    HIP_TRY(h, launch_actor_pack(ac.net, d_weights, const_cast<float *>(ac.net.w), ac.packed, h->stream));
    return GYMNET_OK;
    });
}

int gymnet_vecenv_actor_reset_device(gymnet_vecenv *h, const uint8_t *d_mask) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_actor(h));
    return actor_refill(h, d_mask);
    });
}

int gymnet_vecenv_actor_push_device(gymnet_vecenv *h, const uint8_t *d_done) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_actor(h));
    Actor &ac = *h->actor;
    if (!(since(h, ac.last) == StepMark{1, 1}))
        return fail(h, GYMNET_ERR_INVALID_ARG, "an actor push needs exactly one vector step since the last actor config, reset or push (tick %llu -> %llu, "
                    "%llu step launches, %llu reset / seed / set_tick / set_state calls); after a reset, seed, set_tick or set_state of the handle call "
                    "gymnet_vecenv_actor_reset_device", (unsigned long long)ac.last.tick, (unsigned long long)(h->tick - h->held_ticks),
                    (unsigned long long)since(h, ac.last).launches, (unsigned long long)since(h, ac.last).epoch);   // (ticks on the decision clock: StepMark)
    ActorHist hs = ac.hist;
    hs.slot = ring_next(hs.slot, hs.history);
    HIP_TRY(h, launch_actor_push(h->f64, hs, h->d_obs, h->ostride, d_done ? d_done : h->d_done, true, h->stream));
    ac.hist = hs;
    ac.last = mark(h);
    return GYMNET_OK;
    });
}

int gymnet_vecenv_actor_act_device(gymnet_vecenv *h, int32_t *d_actions, float *d_logits, float epsilon, uint64_t seed, uint64_t tick) {
    return guarded([&]() -> int {
    ENTER(h);
    ActorAct aa;
    ST_TRY(actor_act_enter(h, false, "this handle's actor chooses Box actions: gymnet_vecenv_actor_box_act_device", d_actions, nullptr, epsilon, seed, tick, aa));
    HIP_TRY(h, actor_act_launch(h, d_actions, d_logits, nullptr, aa));
    return GYMNET_OK;
    });
}

int gymnet_vecenv_actor_view(gymnet_vecenv *h, float **d_history, int64_t *lane_stride, int32_t *slot) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_actor(h));
    if (d_history) *d_history = h->actor->hist.hist;
    if (lane_stride) *lane_stride = h->actor->hist.stride;
    if (slot) *slot = h->actor->hist.slot;
    return GYMNET_OK;
    });
}

int gymnet_vecenv_actor_history_device(gymnet_vecenv *h, float *d_out, int64_t out_stride) {
    return guarded([&]() -> int {
    ENTER(h);
    ST_TRY(need_actor(h));
    if (!d_out) return fail(h, GYMNET_ERR_INVALID_ARG, "d_out is null");
    if (!aligned_to(d_out, 4)) return fail(h, GYMNET_ERR_INVALID_ARG, "d_out must be 4-byte aligned");
    if (out_stride < h->n) return fail(h, GYMNET_ERR_INVALID_ARG, "out_stride %lld < num_envs %lld", (long long)out_stride, (long long)h->n);
    if (!actor_current(h))
        return fail(h, GYMNET_ERR_INVALID_ARG, "the actor's history is stale: push after every single vector step (or reset the actor; after a reset, "
                    "seed, set_tick or set_state of the handle only a reset of the actor serves)");
    const ActorHist &hs = h->actor->hist;
    if (hs.n > 0) {
        hipLaunchKernelGGL(actor_history_kernel, lane_grid(hs.n), dim3(256), 0, h->stream, hs, d_out, out_stride);
        HIP_TRY(h, hipGetLastError());
    }
    return GYMNET_OK;
    });
}

}  // extern "C"
