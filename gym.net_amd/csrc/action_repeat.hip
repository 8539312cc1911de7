// action_repeat.hip — frame skip: a decision's action held for R = repeat + 1 env steps inside ONE launch (the reference's
// IGameConfiguration.SkippedFrames, BasePlaySession.cs:37-56).  The contract is gymnet_vecenv_rollout_repeat_device in
// include/gymnet_amd.h.
//
// The kernels are step_kernels.hpp's rollout_body with its HeldAction switch: a trip of the fused rollout's loop is a DECISION — its
// action is chosen once, at the head of the trip — and the part of the body from the env step to the fused reset runs R times, sub-step r
// at engine tick tick0 + d * R + r.  The switch adds the live flag, the decision's reward and done byte and the way back for the next
// sub-step; the env step, the bookkeeping, the record staging and flush, the fused reset and the write-back are the rollout's own.
//
// Builder's choices (every choice computes the same bits):
//   * ONE lane per thread for every env and state scalar.  No alignment rule on any stream, no guarded body (a thread past the end leaves),
//     and the idle test is a branch around the lane's step instead of a select over a second copy of the state.
//   * The per-thread drain reset (RESETF = 0): with one lane per thread a wave pays one Philox pass per sub-step that has a finished lane.
//   * ONE records form: the spill to the shared overflow segment is always compiled (GYMNET_RECORDS_NO_OVERFLOW is a speed hint of the
//     fused rollout; honouring it here would be 24 more kernels for the same records).
//   * No occupancy hint: the fused rollout's (256, 4) bound buys a fourth wave of four-lane threads at the price of scratch; these kernels
//     hold one lane per thread: 143 VGPRs at worst (float64, sampled actions, records), no scratch (profiles/kernel_resources_action_repeat.txt).
// 6 envs x {auto-reset, not} x {lean, bookkeeping, bookkeeping + records} x {ring, sampled} = 72 kernels.
#include "handle.hpp"
#include "envs.hpp"
#include "cartpole64.hpp"
#include "step_kernels.hpp"

namespace gymnet {

// rollout_kernel's prologue (step_kernels.hpp) with one lane per thread and T * R ticks, then rollout_body with the held action
template <class Env, bool AUTORESET, bool EXTRAS, bool SAMPLE, bool RECORDS>
__global__ __launch_bounds__(256) void repeat_rollout_kernel(const StepArgsT<typename Env::Real> a, const RolloutArgsT<typename Env::Real> ro, const int32_t R) {
    static_assert(EXTRAS || !RECORDS, "episode records are a bookkeeping handle's");
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    EpisodeStage *stage = nullptr;
    if constexpr (EXTRAS && RECORDS) {
        __shared__ EpisodeStage stages[256 / 64];                  // one per wave of the workgroup
        stage = &stages[threadIdx.x >> 6];
    }
    const uint64_t tick0 = a.tick2[a.parity];
    if (blockIdx.x == 0 && threadIdx.x == 0) a.tick2[a.parity ^ 1] = tick0 + (uint64_t)ro.steps * (uint64_t)R;
    if constexpr (EXTRAS) {
        if (blockIdx.x == 0 && a.done_count2) {   // zero the NEXT step launch's half of the shard counters (as step_kernel does)
#pragma clang loop vectorize(disable) interleave(disable)
            for (int sh = threadIdx.x; sh < kShards; sh += blockDim.x) a.done_count2[(a.cparity ^ 1) * (kShards * kCountStride) + sh * kCountStride] = 0u;
        }
    }
    // every lane is in range past this line, and the active lanes of the last wave are a prefix (the wave-level helpers rely on it)
    if (i >= a.n) return;
    rollout_body<Env, 1, AUTORESET, false, EXTRAS, SAMPLE, 0, RECORDS ? 1 : 0, NoHook, HeldAction>(a, ro, i, tick0, nullptr, stage, NoHook{}, HeldAction{R});
}

namespace {

template <class Env>
hipError_t launch_repeat_env(bool autoreset, bool extras, const StepArgsT<typename Env::Real> &a, const RolloutArgsT<typename Env::Real> &r, int32_t R,
                             hipStream_t st) {
    using Real = typename Env::Real;
    const bool sample = r.action_source != 0, records = extras && r.ep_lane != nullptr;
    void (*kernel)(StepArgsT<Real>, RolloutArgsT<Real>, int32_t) = nullptr;
    with_bool(autoreset, [&](auto ar) {
        with_bool(extras, [&](auto ex) {
            with_bool(sample, [&](auto smp) {
                with_bool(records, [&](auto rec) {
                    constexpr bool AR = decltype(ar)::value, EX = decltype(ex)::value, SMP = decltype(smp)::value, REC = decltype(rec)::value;
                    if constexpr (EX || !REC) kernel = repeat_rollout_kernel<Env, AR, EX, SMP, REC>;
                });
            });
        });
    });
    if (!kernel) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3(grid_for(a.n > 0 ? a.n : 1, 256)), dim3(256), 0, st, a, r, R);
    return hipGetLastError();
}

}  // namespace

hipError_t repeat_rollout_launch(gymnet_vecenv *h, const StepArgs &a, const RolloutArgs &r, int32_t R) {
    switch (h->cfg.env_id) {
        case GYMNET_ENV_CARTPOLE: return launch_repeat_env<CartPole>(h->autoreset, h->extras, a, r, R, h->stream);
        case GYMNET_ENV_PENDULUM: return launch_repeat_env<Pendulum>(h->autoreset, h->extras, a, r, R, h->stream);
        case GYMNET_ENV_MOUNTAINCAR: return launch_repeat_env<MountainCar>(h->autoreset, h->extras, a, r, R, h->stream);
        case GYMNET_ENV_ACROBOT: return launch_repeat_env<Acrobot>(h->autoreset, h->extras, a, r, R, h->stream);
        case GYMNET_ENV_MOUNTAINCAR_CONTINUOUS: return launch_repeat_env<MountainCarContinuous>(h->autoreset, h->extras, a, r, R, h->stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t repeat_rollout_launch(gymnet_vecenv *h, const StepArgs64 &a, const RolloutArgs64 &r, int32_t R) {
    if (h->cfg.env_id != GYMNET_ENV_CARTPOLE) return hipErrorInvalidValue;   // (the float64 engine is CartPole's)
    return launch_repeat_env<CartPole64>(h->autoreset, h->extras, a, r, R, h->stream);
}

}  // namespace gymnet

// ---- the host side: the entry points, which reach the rollout through rollout_fused_entered (handle.hpp) ---------------------------
using namespace gymnet;

namespace {

bool repeat_in_range(gymnet_vecenv *h, int32_t repeat) {
    if (repeat >= 0 && repeat <= 255) return true;
    fail(h, GYMNET_ERR_INVALID_ARG, "repeat must be in [0, 255] (skipped frames per decision), got %d", repeat);
    return false;
}

// one decision: d_actions held for repeat + 1 env steps (repeat > 0; VALIDATE_ACTIONS has been applied by the caller)
int launch_one_decision(gymnet_vecenv *h, const void *d_actions, int32_t repeat) {
    gymnet_rollout_spec spec{};
    spec.struct_size = sizeof spec;
    spec.action_source = GYMNET_ACTIONS_RING;
    spec.d_actions = d_actions; spec.steps = 1; spec.action_stride = 0; spec.ring = 1;
    return rollout_fused_entered(h, FusedRequest{&spec, repeat, true});
}

}  // namespace

extern "C" {

int gymnet_vecenv_rollout_repeat_device(gymnet_vecenv *h, const gymnet_rollout_spec *spec, int32_t repeat) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!repeat_in_range(h, repeat)) return GYMNET_ERR_INVALID_ARG;
    return rollout_fused_entered(h, FusedRequest{spec, repeat});
    });
}

int gymnet_vecenv_step_repeat_device(gymnet_vecenv *h, const void *d_actions, int32_t repeat) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!repeat_in_range(h, repeat)) return GYMNET_ERR_INVALID_ARG;
    if (!d_actions) return fail(h, GYMNET_ERR_INVALID_ARG, "d_actions is null");
    if (repeat == 0 && h->lcfg.vec > 1 && !aligned_to(d_actions, 4 * h->lcfg.vec))
        return fail(h, GYMNET_ERR_INVALID_ARG, "d_actions must be %d-byte aligned", 4 * h->lcfg.vec);
    ST_TRY(validate_staged_actions(h, d_actions));
    return repeat == 0 ? launch_one_step(h, d_actions) : launch_one_decision(h, d_actions, repeat);
    });
}

int gymnet_vecenv_step_repeat(gymnet_vecenv *h, const void *actions, int32_t repeat, void *obs_out, float *reward_out, uint8_t *done_out) {
    return guarded([&]() -> int {
    ENTER(h);                            // (not served by the resident kernel: a resident handle leaves residency first)
    if (h->async_pending) return fail(h, GYMNET_ERR_ALREADY_STEPPING, "already running an async step");
    if (!repeat_in_range(h, repeat)) return GYMNET_ERR_INVALID_ARG;
    const void *d_act = nullptr;
    ST_TRY(stage_host_actions(h, actions, &d_act, true));
    ST_TRY(repeat == 0 ? launch_one_step(h, d_act) : launch_one_decision(h, d_act, repeat));
    return copy_out(h, obs_out, reward_out, done_out);
    });
}

}  // extern "C"
