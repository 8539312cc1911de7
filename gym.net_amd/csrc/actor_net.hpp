// actor_net.hpp — what the eight actor units share: the network and the per-lane observation history as the kernels see them, the forward
// pass, the ring arithmetic, the push (as a kernel and as the `after` half of rollout_body's hook), the host helpers every unit launches
// with (lane_grid, pick_rollout_form), and the handle's Actor attachment with each unit's launch calls.  actor.hip serves the Discrete
// envs (argmax head) and owns the attachment, the act prologue (actor_act_enter) and the router: actor_rollout_launch there is the one
// place that says which unit runs a handle's fused rollout, and no unit calls another on its own.  actor_box.hip serves the Box envs
// (clamp head), actor_box_policy.hip their other policies (tanh head, Gaussian noise), actor_box_logd.hip the Box envs when the caller also
// asks for the log-density of the action taken or, inside the rollout, the critic's value, actor_softmax.hip the Discrete envs under an
// exploration setting other than the default (a draw from the softmax of the logits), actor_logp.hip the Discrete envs when the caller
// also asks for the log-probability of the action taken, actor_value.hip the critic: a second network over the same input whose one
// output is the lane's value estimate, actor_boot.hip either kind when the caller also asks for the critic's value of the terminal
// observation on time-limit rows.  Internal to the library.
#pragma once
#include "step_kernels.hpp"

#include "envs.hpp"
#include "handle.hpp"

namespace gymnet {

// a fully connected ReLU network of `layers` linear layers whose packed weights (actor_net_shape) are read by every lane, and the
// per-lane observation history it reads
constexpr int kActorMaxLayers = 4, kActorMaxWidth = 64, kActorMaxParams = 8192, kActorMaxActions = 8;
struct ActorNet {
    const float *w;                            // packed block: layer l at w + off[l] (actor_forward)
    int32_t layers, action_n;                  // action_n: the last layer's width (the Discrete space's n; 1 for a Box actor)
    int32_t win[kActorMaxLayers], wout[kActorMaxLayers], off[kActorMaxLayers];
};
struct ActorHist {
    float *hist; int64_t stride;               // [history][obs_dim][stride] float32, a ring
    int32_t history, obs_dim;
    int32_t slot;                              // ring slot of the newest observation (push: the slot this push writes)
    int64_t n;
};
struct ActorAct { float epsilon; uint64_t seed, lane_offset, tick; };

typedef __attribute__((address_space(4))) const float cfloat;   // scalar-cache (constant address space) view of the weights

constexpr int kW = kActorMaxWidth;

// Layer l of the packed block: ceil(wout / 4) groups of [4 biases | ceil(win / 8) chunks of [4 rows][8 inputs]], zeros where a row or
// an input does not exist.
__host__ __device__ __forceinline__ int64_t group_floats(int32_t win) { return 4 + 32 * (int64_t)((win + 7) >> 3); }

// x: the input layer's activations, +0 beyond net.win[0]; on return x[0 .. action_n) are the last layer's values
__device__ __forceinline__ void actor_forward(const ActorNet &net, float (&x)[kW]) {
    for (int l = 0; l < net.layers; ++l) {                                   // wave-uniform
        const int32_t win = net.win[l], wout = net.wout[l];
        const int32_t nch = (win + 7) >> 3;
        const bool hidden = l + 1 < net.layers;
        const int64_t gf = group_floats(win);
        cfloat *wl = (cfloat *)(net.w + net.off[l]);
        float y[kW];
#pragma unroll
        for (int g = 0; g < kW / 4; ++g) {
            float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (4 * g < wout) {                                              // wave-uniform
                cfloat *blk = wl + g * gf;
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) acc[jj] = blk[jj];
#pragma unroll
                for (int c = 0; c < kW / 8; ++c) {
                    if (c < nch) {                                           // wave-uniform
                        cfloat *ch = blk + 4 + 32 * c;
#pragma unroll
                        for (int ii = 0; ii < 8; ++ii) {
#pragma unroll
                            for (int jj = 0; jj < 4; ++jj) acc[jj] = __builtin_fmaf(ch[jj * 8 + ii], x[8 * c + ii], acc[jj]);
                        }
                    }
                }
                if (hidden) {
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) acc[jj] = acc[jj] > 0.0f ? acc[jj] : 0.0f;
                }
            }
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) y[4 * g + jj] = acc[jj];
        }
#pragma unroll
        for (int i = 0; i < kW; ++i) x[i] = y[i];
    }
}

// first index of the largest of x[0 .. action_n) (moves only on a strictly greater value), which also hands out the value it settles on:
// actor.hip's argmax_logits as actor_softmax.hip and actor_logp.hip need it
__device__ __forceinline__ int32_t argmax_value(const float (&x)[kW], int32_t action_n, float &bv) {
    int32_t best = 0;
    bv = x[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) {
        if (j < action_n && x[j] > bv) { bv = x[j]; best = j; }
    }
    return best;
}

// the ring: the slot after `slot`, and the slot of input row s (oldest first, s < history) when `newest` holds the newest observation
__host__ __device__ __forceinline__ int32_t ring_next(int32_t slot, int32_t history) { return slot + 1 == history ? 0 : slot + 1; }
__device__ __forceinline__ int32_t ring_row(int32_t newest, int32_t s, int32_t history) {
    int32_t row = newest + 1 + s;
    row = row >= history ? row - history : row;
    row = row >= history ? row - history : row;
    return row;
}

// the network input of lane i: ring slots oldest first, O values each (O compile-time, so x's indices are)
template <int O>
__device__ __forceinline__ void load_input(const ActorHist &hs, int32_t newest, int64_t i, float (&x)[kW]) {
#pragma unroll
    for (int s = 0; s < kW / O; ++s) {
        int32_t row = 0;
        if (s < hs.history) row = ring_row(newest, s, hs.history);           // wave-uniform
#pragma unroll
        for (int k = 0; k < O; ++k) x[s * O + k] = s < hs.history ? hs.hist[((int64_t)row * O + k) * hs.stride + i] : 0.0f;
    }
#pragma unroll
    for (int i2 = (kW / O) * O; i2 < kW; ++i2) x[i2] = 0.0f;
}

// one lane's push: the new slot only in the common case, every slot for a lane that restarts.  v is loaded before any store (the history
// is not declared apart from it, so a load after a store of the ring would be issued again behind that store)
template <int O>
__device__ __forceinline__ void push_lane(const ActorHist &hs, int32_t slot, int64_t i, bool all, const float (&v)[O]) {
    float *__restrict__ h = hs.hist + i;
    if (!all) {                                       // the common case: one slot
#pragma unroll
        for (int k = 0; k < O; ++k) h[((int64_t)slot * O + k) * hs.stride] = v[k];
        return;
    }
    for (int sl = 0; sl < hs.history; ++sl) {
#pragma unroll
        for (int k = 0; k < O; ++k) h[((int64_t)sl * O + k) * hs.stride] = v[k];
    }
}

// push (restart = done bytes; lanes without one write the new slot only) or fill (restart = mask, NULL: every lane; lanes without one
// are not touched)
template <class R, int O>
__global__ __launch_bounds__(256) void actor_push_kernel(const ActorHist hs, const R *__restrict__ obs, int64_t obs_stride,
                                                         const uint8_t *__restrict__ restart, int32_t push) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hs.n) return;
    const bool all = restart ? restart[i] != 0 : !push;
    if (!push && !all) return;
    float v[O];
#pragma unroll
    for (int k = 0; k < O; ++k) v[k] = (float)obs[k * obs_stride + i];
    push_lane<O>(hs, hs.slot, i, all, v);
}

// the `after` half of rollout_body's hook (step_kernels.hpp), one lane per thread: gymnet_vecenv_actor_push_device as actor_push_kernel
// does it, with the post-step observation taken from the rollout's registers.  newest: the ring slot of the newest observation, moved on
template <class Env>
__device__ __forceinline__ void hook_push(const ActorHist &hs, int32_t &newest, int64_t i, const uint8_t (&done)[1], const float (&s)[Env::S][1],
                                          const float (&o)[Env::O][1]) {
    constexpr int S = Env::S, O = Env::O;
    newest = ring_next(newest, hs.history);
    float v[O];
#pragma unroll
    for (int k = 0; k < O; ++k) v[k] = Env::OBS_ALIASES_STATE ? s[k < S ? k : 0][0] : o[k][0];
    push_lane<O>(hs, newest, i, done[0] != 0, v);
}

// kActorMinBlocks: the lean forms fit three waves per SIMD (three workgroups of four waves per CU, 168 VGPRs) and are held to it — one
// register more would cost a third of their occupancy; the bookkeeping forms (181-207 VGPRs, two waves) get no cap: 1 is the default.
template <bool EXTRAS> constexpr int kActorMinBlocks = EXTRAS ? 1 : 3;

static inline dim3 lane_grid(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// a fused rollout's three run-time switches as compile-time ones: f(AUTORESET, EXTRAS, RECORDS), each a std::bool_constant, for the six
// forms every unit compiles.  Records without the bookkeeping is not a form: the lean kernel runs
template <class F>
auto pick_rollout_form(bool autoreset, bool extras, bool records, F f) {
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    if (autoreset) {
        if (!extras) return f(yes, no, no);
        return records ? f(yes, yes, yes) : f(yes, yes, no);
    }
    if (!extras) return f(no, no, no);
    return records ? f(no, yes, yes) : f(no, yes, no);
}

// the configured actor: hist.slot is the ring slot of the newest observation; last: the handle's step counters at the last config, reset,
// push or actor rollout, so act can tell that the history is current and push that exactly one vector step ran in between.  box: the
// handle's env has a Box action space and the last layer's one value is the action (actor_box.hip); else its values are logits
struct Actor {
    DeviceAllocs mem; ActorNet net{}; ActorHist hist{}; int64_t count = 0, packed = 0; StepMark last; bool box = false;
    // a Box actor's policy (gymnet_vecenv_actor_box_set_policy): a fresh actor has the default, which the kernels of actor_box.hip serve;
    // any other runs through actor_box_policy.hip
    int32_t head = GYMNET_BOX_HEAD_CLAMP, explore = GYMNET_BOX_EXPLORE_SAMPLE; float sigma = 0.0f;
    bool default_policy() const { return head == GYMNET_BOX_HEAD_CLAMP && explore == GYMNET_BOX_EXPLORE_SAMPLE; }
    // a Discrete actor's exploration setting (gymnet_vecenv_actor_set_exploration): a fresh actor has the default, which the kernels of
    // actor.hip serve (UNIFORM at any temperature is that behaviour); SOFTMAX runs through actor_softmax.hip.  inv_tau = 1.0f / temperature
    int32_t discrete_explore = GYMNET_ACTOR_EXPLORE_UNIFORM; float temperature = 1.0f, inv_tau = 1.0f;
    bool default_exploration() const { return discrete_explore == GYMNET_ACTOR_EXPLORE_UNIFORM; }
    // the critic (gymnet_vecenv_actor_critic_config, actor_value.hip): a second network over the same input, last width 1, in an
    // allocation of its own so that it comes and goes without the actor; critic.layers == 0: none
    DeviceAllocs critic_mem; ActorNet critic{}; int64_t critic_count = 0, critic_packed = 0;
    bool has_critic() const { return critic.layers > 0; }
};
// what the kernels of actor_box_policy.hip take of it, as a kernel argument
struct BoxPolicy { int32_t head, explore; float sigma; };
inline BoxPolicy box_policy(const Actor &ac) { return {ac.head, ac.explore, ac.sigma}; }
// ... and the kernels of actor_softmax.hip and actor_logp.hip
struct ActorExplore { int32_t explore; float inv_tau; };
inline ActorExplore actor_explore(const Actor &ac) { return {ac.discrete_explore, ac.inv_tau}; }

// the message names the config call that serves the handle's env
inline int need_actor(gymnet_vecenv *h) {
    return h->actor ? GYMNET_OK : fail(h, GYMNET_ERR_INVALID_ARG, kNoActorFormat, actor_config_call(h->desc->box_action));   // (rollout_plan.hpp)
}

// the history is current: no vector step since the last actor config, reset, push or actor rollout
inline bool actor_current(const gymnet_vecenv *h) { return since(h, h->actor->last) == StepMark{0, 0}; }

// actor.hip: gymnet_vecenv_actor_config and gymnet_vecenv_actor_box_config behind ENTER (box: which of the two)
int actor_configure(gymnet_vecenv *h, bool box, int32_t history, int32_t num_layers, const int32_t *widths, const float *weights, int64_t count);
// actor.hip: what both config calls and the critic's check of a network's shape once num_layers and the pointers are known good — every
// width, the first (history * obs_dim) and the last (`last`, worded `last_name`), the parameter limit and count — with nothing changed on a
// refusal, and then make of it: the ActorNet of these widths (w unset) and its packed size; flat device weights -> the packed block
int actor_net_check(gymnet_vecenv *h, int32_t num_layers, const int32_t *widths, int64_t count, int32_t first, int32_t last, const char *last_name,
                    int64_t &params);
int64_t actor_net_shape(ActorNet &net, int32_t num_layers, const int32_t *widths);
hipError_t launch_actor_pack(const ActorNet &net, const float *flat, float *packed, int64_t packed_count, hipStream_t st);
// actor.hip: what every act entry point checks behind ENTER, in this order — an actor of the kind the call serves (want_box; wrong_kind:
// the entry point's own message), d_actions, d_logp's alignment (null: not asked for), epsilon, a current history — and the ActorAct of
// the launch
int actor_act_enter(gymnet_vecenv *h, bool want_box, const char *wrong_kind, const void *d_actions, const float *d_logp, float epsilon, uint64_t seed,
                    uint64_t tick, ActorAct &aa);
// Each unit's fused rollout of a handle it serves, a.n > 0 (records: the rollout keeps compact episode records), and the calls one unit
// makes into another: actor.hip's router (actor_rollout_launch, handle.hpp) reads (box, default_policy(), default_exploration(), a record
// pointer) and calls exactly one of these eight or its own unit's; the act entry points of actor.hip and actor_box.hip and actor.hip's
// push reach a sibling's kernels through the rest.
// actor_box.hip: the default policy's rollout, and the push / fill of a three-row observation (Pendulum)
hipError_t actor_box_rollout_launch(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r);
hipError_t launch_actor_box_push3(const ActorHist &hs, const float *obs, int64_t obs_stride, const uint8_t *restart, bool push, hipStream_t st);
// actor_box_policy.hip: a Box handle whose policy is not the default
hipError_t actor_box_policy_rollout_launch(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r);
hipError_t actor_box_policy_act_launch(const ActorNet &net, const ActorHist &hs, float *actions, float *raw, float low, float high, const ActorAct &aa,
                                       const BoxPolicy &pol, hipStream_t st);
// actor_box_logd.hip: a Box handle, any policy with sigma > 0, that records the log-density of every action taken (rec_logd [steps][n]) and
// / or, with a critic, the value of every step's input (rec_value [steps][n]); either may be null
hipError_t actor_box_logd_rollout_launch(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r, float *rec_logd, float *rec_value);
// actor_softmax.hip: a Discrete handle whose exploration setting is not the default
hipError_t actor_softmax_rollout_launch(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r);
hipError_t actor_softmax_act_launch(const ActorNet &net, const ActorHist &hs, int32_t *actions, float *logits, const ActorAct &aa, const ActorExplore &ex,
                                    hipStream_t st);
// actor_logp.hip: a Discrete handle, either setting, that also records the log-probability of every action taken: rec_logp [steps][n]
hipError_t actor_logp_rollout_launch(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r, float *rec_logp);
hipError_t actor_logp_act_launch(const ActorNet &net, const ActorHist &hs, int32_t *actions, float *logits, float *logp, const ActorAct &aa,
                                 const ActorExplore &ex, hipStream_t st);
// actor.hip: act on a Discrete handle, by the unit that serves it as it stands (logp null: none asked for)
hipError_t actor_act_launch(gymnet_vecenv *h, int32_t *actions, float *logits, float *logp, const ActorAct &aa);
// actor_value.hip: a Discrete handle with a critic, either setting, that records the critic's value of every step's input: rec_value
// [steps][n], and the log-probabilities as above where rec_logp is not null
hipError_t actor_value_rollout_launch(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r, float *rec_logp, float *rec_value);
// actor_boot.hip: either kind with a critic on a handle with a time limit (a bookkeeping handle), that records the values as above and
// V(terminal observation) on time-limit rows: rec_boot [steps][n]; rec_logp / rec_logd may be null
hipError_t actor_value_boot_rollout_launch(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r, float *rec_logp, float *rec_value,
                                           float *rec_boot);
hipError_t actor_box_boot_rollout_launch(gymnet_vecenv *h, bool records, const StepArgs &a, const RolloutArgs &r, float *rec_logd, float *rec_value,
                                         float *rec_boot);

}  // namespace gymnet
