// kernels.hpp — launch interface between the C-ABI layer (capi.hip) and the HIP kernels (kernels.hip, env_*.hip).  The attachment units
// (render.hip, pixel_stack.hip, episode_memory.hip, actor.hip) keep their kernels' argument structs and launchers to themselves.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch_policy.hpp"
#include "rollout_plan.hpp"

namespace gymnet {

// Everything one vector-step launch needs.  Passed by value (kernarg segment).
// R is the STATE SCALAR of the handle: float (the batched engine's structure-of-arrays hot path) or double (GYMNET_FLAG_F64: the
// reference's own arithmetic, CartPoleEnv.cs:141-166,185 — float64 state that IS the float64 observation).  Everything that holds a
// state or observation value is typed R; reward (Step.cs:9: a C# float), done, the actions and all counters are the same for both.
template <class R>
struct StepArgsT {
    R *state;                // [S][state_stride]  structure-of-arrays, one env per lane (read)
    R *state_out;            // where the new state is written: == state, or the OTHER half of a double-buffered pair
                             // (GYMNET_FLAG_DOUBLE_BUFFER: step t+1 writes B while a gather of A is still in flight)
    R *obs;                  // [O][obs_stride]    (unused when the env's observation aliases its state)
    const R *obs_in;         // the CURRENT observation buffer (== obs unless double-buffered): state rows the observation repeats
                             // (Env::OBS_ROW_OF_STATE) are read from here — they have no row of their own in `state`
    const void *action;      // int32[n] (Discrete) or float32[n] (Box)
    float *reward;           // [n]
    uint8_t *done;           // [n]
    int32_t *sbd;            // [n] CartPole steps_beyond_done (CartPoleEnv.cs:41); NULL with auto-reset
    uint64_t *tick2;         // device tick, double-buffered: launch with tick t reads tick2[t&1], writes tick2[(t+1)&1]=t+1
    // extras (all NULL / 0 in the lean hot-path variant)
    R *final_obs;            // [O][n] dense terminal observations; NULL = none kept / compact records only
    // Done-lane compaction is SHARDED: 4096 waves hammering one counter word serialise at ~88 atomics/us (46 us per
    // step at 2^20 lanes, measured); wave w appends to shard w % kShards, each shard has its own counter (64-byte
    // stride) and its own segment of the list.  compact_done gathers the segments into one list on demand.
    int32_t *done_list;      // [kShards][done_cap] segmented
    uint32_t *done_count2;   // [2][kShards * kCountStride]: this launch fills half [cparity] and zeroes half [cparity^1]
    int64_t done_cap;        // entries per shard segment
    float *ep_ret; int32_t *ep_len;
    float *fin_ret; int32_t *fin_len;   // dense last-finished-episode arrays; NULL = compact records only (with done_list)
    // compact records, segmented like done_list (position p of shard s = the lane at done_list[s * done_cap + p]):
    float *rec_ret; int32_t *rec_len;   // [kShards][done_cap]     finished episode's return / length   (EPISODE_STATS + DONE_LIST)
    R *rec_obs;                         // [kShards][O][done_cap]  terminal observation                  (FINAL_OBS + DONE_LIST)
    const uint64_t *lane_seed;       // [n] per-lane Philox keys (VecEnv.Seed(int[])) or NULL
    unsigned long long *after_done;  // [kShards * kAfterStride] sharded counter: steps taken on already-done lanes (CartPoleEnv.cs:176-179)
    int64_t n, state_stride, obs_stride;
    uint64_t lane_offset, seed;
    int32_t parity;          // tick & 1 of this launch
    int32_t cparity;         // (number of step launches so far) & 1: which done_count2 slot this launch fills
    int32_t max_episode_steps;
};
typedef StepArgsT<float> StepArgs;
typedef StepArgsT<double> StepArgs64;

// How the one-step kernels (step_kernel, step_kernel_pipe, step_kernel_pipe2) receive a StepArgsT: its FIRST-USE words as flat leading
// arguments, the whole struct behind them.  gfx950 delivers up to 14 dwords of flat leading kernel arguments in user SGPRs at wave
// launch (-mllvm -amdgpu-kernarg-preload-count=14, gym.net_amd/build.py) — a by-value struct is never preloaded — so what the guard,
// the first vector loads and the tick load need is there before the first instruction, with no scalar load from the kernarg segment
// and no wait for one (profiles/launch_floor.txt).  The words, by first use: state, action, n, state_stride (the guard and the loads),
// tick2 and parity (the tick load), reward (the first stream stored), and `block`, the launch's workgroup size: blockDim.x is a HIDDEN
// kernel argument, which is preloaded only when every explicit argument is, so the kernels read it from here.  The kernel rebuilds its
// StepArgsT from `rest` and the flat words (step_kernels.hpp hot_step_args); launch_step_kernel is the one place that splits it.
template <class R>
using StepKernelFn = void (*)(R *state, const void *action, int64_t n, int64_t state_stride, uint64_t *tick2, float *reward, int32_t block,
                              int32_t parity, StepArgsT<R> rest);

// (kShards, kCountStride: rollout_plan.hpp, whose EpisodeSegments lays a rollout's episode records out by them)
constexpr int kAfterStride = 8;     // uint64 words between after_done shards (64 bytes)
// (LaunchCfg, a launch's configuration, and the rules that choose a handle's first one: launch_policy.hpp)

// Fused multi-step rollout: `steps` vector steps inside ONE launch; state stays in registers between steps.
// Round 5: the rollout carries what its consumer needs (examples/.../PlaySessions/BasePlaySession.cs:58-69 accumulates the episode
// reward and keeps the best episodes, MemoryTypes/ReplayMemory.cs:53-67; TrainingPlaySession.cs:46-52 draws epsilon-greedy actions
// per step): on a bookkeeping handle the running episode return / length live in registers, max_episode_steps truncates, per-lane
// seeds key the reset draws, and every finished episode leaves a compact (t, lane, return, length) record; and the actions can be
// DRAWN IN THE KERNEL — the words sample_discrete_kernel / compose_discrete_kernel would produce for (action_seed, action_tick0 + t)
// — so a random or epsilon-greedy rollout reads no action ring at all.
template <class R>
struct RolloutArgsT {
    int64_t steps;           // T
    int64_t action_stride;   // elements between consecutive action slices
    int64_t ring;            // step t reads slice t % ring
    R *rec_obs;              // optional [T][O][n]   (NULL = do not record)
    float *rec_reward;       // optional [T][n]
    uint8_t *rec_done;       // optional [T][n]
    void *rec_action;        // optional [T][n] the actions TAKEN (int32 / float32): what a replay memory stores beside obs / reward / done
    // action source: 0 = the ring (StepArgs::action); 1 = ActionSpace.Sample() per lane and step; 2 = epsilon-greedy — with
    // probability epsilon the sampled action, else the ring's (policy) action.  Philox action stream, counter (global lane, action_tick0 + t).
    int32_t action_source;
    float epsilon;
    uint64_t action_seed, action_tick0;
    // compact episode records of the WHOLE rollout, segmented like StepArgs::done_list: wave w appends to shard w % kShards
    // (ep_count[shard * kCountStride], one atomic per wave and step that has a finished lane), record p of shard s at s * ep_cap + p
    int32_t *ep_t, *ep_lane;      // step index inside the rollout, lane
    float *ep_ret; int32_t *ep_len;
    uint32_t *ep_count;           // [kShards * kCountStride], zeroed by the launcher; counts beyond ep_cap go to the overflow segment
    int64_t ep_cap;
    // Round 6: ONE overflow segment shared by all shards, for the records a shard's own segment cannot hold (lanes that finish
    // unevenly: a few waves producing most of the episodes).  It is "segment kShards" of the same four arrays — record p at
    // kShards * ep_cap + p, its counter at ep_count[kShards * kCountStride] — so the kernel needs no pointers of its own for it (the
    // rollout kernels are short of scalar registers: six more argument words cost the records variant 0.5 us per vector step).  The
    // counter counts every overflowed record; the first ov_cap are kept.  ov_cap = the caller's ep_capacity: records are dropped only
    // beyond ep_capacity in TOTAL.  records_no_overflow (GYMNET_RECORDS_NO_OVERFLOW): the kernel variant without the spill path.
    int64_t ov_cap;
    int32_t records_no_overflow;
};
typedef RolloutArgsT<float> RolloutArgs;
typedef RolloutArgsT<double> RolloutArgs64;

template <class R>
struct ResetArgsT {
    R *state; R *obs; int32_t *sbd; uint8_t *done;   // done flags cleared for reset lanes
    const uint8_t *mask;      // NULL = all lanes
    uint64_t *tick2; const uint64_t *lane_seed;
    float *ep_ret; int32_t *ep_len;
    int64_t n, state_stride, obs_stride;
    uint64_t lane_offset, seed;
    int32_t parity;
};
typedef ResetArgsT<float> ResetArgs;
typedef ResetArgsT<double> ResetArgs64;

// ---- resident single-wave kernel (GYMNET_FLAG_RESIDENT; N <= 64 lanes: the single-instance facade's latency path) -----------------
// The reference's usage shape is ONE env stepped in a host loop (README.md:32-52, Env.cs:13-41).  Served by one kernel launch +
// one stream synchronize per step that costs ~25 us; served by a RESIDENT kernel — one wave that stays on the GPU, polls a mailbox
// in page-locked, device-mapped, coherent HOST memory for commands and writes observation / reward / done back into it — a step
// is two PCIe crossings and no launch.  The kernel leaves by itself after `idle_polls` polls without a command (or on the exit
// command) and touches nothing afterwards; the host restarts it on the next command.  Same per-lane code (step_body / reset_lane)
// and Philox counters as the launch path: bit-identical.
constexpr int kMailboxLanes = 64;
struct Mailbox {
    uint64_t cmd_seq;                 // host -> device: sequence number of the newest command (the host writes it LAST, release)
    uint32_t cmd;                     // kMailboxStep / ResetAll / ResetDone / Exit
    uint32_t pad0;
    uint64_t done_seq;                // device -> host: the last command whose results are in the mailbox (written LAST, release)
    uint32_t exited;                  // device -> host: the kernel has left; it touches nothing afterwards
    uint32_t pad1;
    uint64_t tick;                    // device -> host: engine tick after the last command
    uint64_t pad2[3];
    int32_t actions[kMailboxLanes];   // int32 (Discrete) or float32 bits (Box), one per lane
    float reward[kMailboxLanes];
    uint8_t done[kMailboxLanes];
    // the observations follow at kMailboxObsOffset: row-major [lane][obs_dim] of the handle's state scalar (<= 64 * 6 * 8 bytes)
};
constexpr size_t kMailboxObsOffset = 1024;
constexpr size_t kMailboxBytes = kMailboxObsOffset + (size_t)kMailboxLanes * 8 * 8;
static_assert(sizeof(Mailbox) <= kMailboxObsOffset, "mailbox header overlaps the observations");
constexpr uint32_t kMailboxStep = 1, kMailboxResetAll = 2, kMailboxResetDone = 3, kMailboxExit = 4;

// ---- env-dependent launchers: one table per env and state scalar (step_kernels.hpp launchers_of, instantiated by env_*.hip) -----

// The step kernel instantiation a launch configuration resolves to (step_kernels.hpp select_step): launch_step_env launches exactly
// this, and gymnet_vecenv_kernel_name / the resolved launch shape read the same decision.
struct StepForm {
    int vec = 1;           // lanes per thread on the wide accesses
    int sequential = 1;    // lanes (or lane pairs) a thread works through one after another in the multi-lane forms (1 = one-shot)
    int slices = 1;        // > 1: the step is that many launches over consecutive slices of the batch (step_kernels.hpp pipe2_chunks)
    int (*text)(char *buf, size_t cap, int slices) = nullptr;
    // the instantiation as text ("step_kernel<CartPole,4,true,false,15,1>", " x G" for G slices); snprintf's contract
    int name(char *buf, size_t cap) const { return text(buf, cap, slices); }
};
template <class R>
struct StepKernelT : StepForm {
    StepKernelFn<R> kernel = nullptr;                      // step_kernel / step_kernel_pipe / step_kernel_pipe2, or
    void (*lds_kernel)(StepArgsT<R>, int64_t) = nullptr;   // step_kernel_lds (its second argument: the batch's 512-lane tiles)
    dim3 grid, block;                                      // the launch over the whole batch
    size_t lds_bytes = 0;                                  // dynamic LDS
    int64_t slice_lanes = 0, group_lanes = 0;              // slices > 1: lanes per slice, lanes per workgroup
};

template <class R>
struct EnvLaunchers {
    // one vector step (autoreset / extras select the compiled variant)
    hipError_t (*step)(bool autoreset, bool extras, const StepArgsT<R> &a, LaunchCfg cfg, hipStream_t st);
    // what `step` runs for this configuration; n: the batch size (one form needs whole 2 * items * 256-lane groups)
    StepKernelT<R> (*select_step)(bool autoreset, bool extras, LaunchCfg cfg, int64_t n);
    // Same results as `steps` step calls (bitwise) — with r.action_source != 0: as `steps` x (sample / compose actions, then step).
    hipError_t (*rollout)(bool autoreset, bool extras, const StepArgsT<R> &a, const RolloutArgsT<R> &r, LaunchCfg cfg, hipStream_t st);
    hipError_t (*reset)(const ResetArgsT<R> &a, hipStream_t st);
    // starts the resident kernel of a small handle (a.n <= kMailboxLanes; a.action must point at mb->actions); mb: device-visible address
    hipError_t (*resident)(bool autoreset, bool extras, const StepArgsT<R> &a, const ResetArgsT<R> &r, Mailbox *mb, uint64_t idle_polls,
                           hipStream_t st);
    // recompute obs from state (after set_state) for envs whose observation is derived; nothing for the others
    hipError_t (*observe)(const R *state, int64_t sstride, R *obs, int64_t ostride, int64_t n, hipStream_t st);
};
// one per env_*.hip (functions, not global tables: clang would copy a constant global table into the device code object too)
const EnvLaunchers<float> &cartpole_launchers();
const EnvLaunchers<float> &pendulum_launchers();
const EnvLaunchers<float> &mountaincar_launchers();
const EnvLaunchers<float> &acrobot_launchers();
const EnvLaunchers<float> &mountaincar_continuous_launchers();
const EnvLaunchers<double> &cartpole64_launchers();   // GYMNET_FLAG_F64: CartPole in the reference's own binary64 arithmetic

// Number of gymnet_env_id values: every env id range check and the per-env tables (capi.hip kEnvs, env_launchers) use it.
constexpr int kNumEnvs = 5;

// The launchers of env `env_id` (gymnet_env_id) in state scalar R (float, or double for the float64 engine); NULL: no such env, or no
// float64 form of it (the reference defines float64 arithmetic for CartPole only).  kernels.hip.
template <class R>
const EnvLaunchers<R> *env_launchers(int env_id);

// Gathers the kShards segments of a fused rollout's episode records (RolloutArgs::ep_*) into compact arrays out_*[0 .. *out_count);
// records beyond out_capacity are dropped, the count is the number of records kept by the rollout.  Any out array may be NULL.
struct EpisodeGatherArgs {
    const uint32_t *counts; int64_t cap;
    const int32_t *ep_t, *ep_lane; const float *ep_ret; const int32_t *ep_len;
    int64_t ov_cap;                // the shared overflow segment = segment kShards of the same arrays (RolloutArgs)
    int32_t *out_t, *out_lane; float *out_ret; int32_t *out_len;
    int64_t out_capacity; uint32_t *out_count;
};
hipError_t launch_gather_episodes(const EpisodeGatherArgs &a, hipStream_t st);

// observations: SoA [O][stride] -> row-major [n][O]; float32, or float64 for a GYMNET_FLAG_F64 handle (here and below)
hipError_t launch_pack_obs(int obs_dim, const float *obs, int64_t stride, float *out_rowmajor, int64_t n, hipStream_t st);
hipError_t launch_pack_obs(int obs_dim, const double *obs, int64_t stride, double *out_rowmajor, int64_t n, hipStream_t st);
// small batches at the host boundary: obs (row-major), reward and done written straight into ONE host-mapped buffer
// [n*O floats | n floats | n bytes] by a single kernel — no device-to-host memcpy calls on the latency path
hipError_t launch_export_small(int obs_dim, const float *obs, int64_t stride, const float *reward, const uint8_t *done,
                               float *out_obs, float *out_reward, uint8_t *out_done, int64_t n, hipStream_t st);
hipError_t launch_export_small(int obs_dim, const double *obs, int64_t stride, const float *reward, const uint8_t *done,
                               double *out_obs, float *out_reward, uint8_t *out_done, int64_t n, hipStream_t st);
// any batch size: obs (row-major), reward, done written straight into page-locked device-mapped HOST memory (the stores are the
// PCIe transfer); any out pointer may be NULL
hipError_t launch_export_host(int obs_dim, const float *obs, int64_t stride, const float *reward, const uint8_t *done,
                              float *out_obs, float *out_reward, uint8_t *out_done, int64_t n, hipStream_t st);
hipError_t launch_export_host(int obs_dim, const double *obs, int64_t stride, const float *reward, const uint8_t *done,
                              double *out_obs, float *out_reward, uint8_t *out_done, int64_t n, hipStream_t st);
hipError_t launch_fill_i32(int32_t *p, int32_t v, int64_t n, hipStream_t st);
// Gathers the sharded done list of one step (counter half `counts`) and the records written beside it into compact arrays
// out_*[0 .. *out_count) (entries beyond out_capacity are dropped; the count is the true one), and / or applies the records to
// the dense per-lane arrays.  Every out / dense / rec pointer may be NULL.
template <class R>
struct CompactArgsT {
    const uint32_t *counts; const int32_t *list; int64_t cap;
    const float *rec_ret; const int32_t *rec_len; const R *rec_obs; int32_t obs_dim;
    int32_t *out_list; float *out_ret; int32_t *out_len; R *out_obs;       // out_obs: row-major [count][obs_dim]
    int64_t out_capacity;
    uint32_t *out_count;
    float *dense_ret; int32_t *dense_len; R *dense_obs; int64_t n;         // dense_obs: [obs_dim][n]
};
typedef CompactArgsT<float> CompactArgs;
hipError_t launch_compact_done(const CompactArgsT<float> &a, hipStream_t st);
hipError_t launch_compact_done(const CompactArgsT<double> &a, hipStream_t st);
// counts actions outside [0, nvals) into *bad
hipError_t launch_validate_discrete(const int32_t *a, int64_t n, int32_t nvals, uint32_t *bad, hipStream_t st);
hipError_t launch_sample_discrete(int32_t *out, int64_t n, int32_t nvals, int32_t start, uint64_t seed,
                                  uint64_t lane_offset, uint64_t tick, hipStream_t st);
// Discrete.Sample(mask) (Discrete.cs:18-26): mask uint8 [n][nvals] (mask_stride = nvals) or one row for every lane (mask_stride = 0)
hipError_t launch_sample_discrete_masked(int32_t *out, int64_t n, int32_t nvals, int32_t start, const uint8_t *mask,
                                         int64_t mask_stride, uint64_t seed, uint64_t lane_offset, uint64_t tick, hipStream_t st);
// Direct all-gather, push form: copies `count` 4-byte words (floats; a float64 slice counts two per element) from src to the same offset inside each of `npeers` peer buffers
// (peer-mapped device memory reached over xGMI, or buffers on the same device for logical shards).
constexpr int kMaxPeers = 15;
struct PushArgs { const float *src; float *dst[kMaxPeers]; int64_t count; int32_t npeers; };
hipError_t launch_push_obs(const PushArgs &a, hipStream_t st);
hipError_t launch_compose_discrete(const int32_t *policy, int32_t *out, int64_t n, int32_t nvals, float epsilon, uint64_t seed,
                                   uint64_t lane_offset, uint64_t tick, hipStream_t st);
hipError_t launch_sample_box(float *out, int64_t n, float low, float high, uint64_t seed, uint64_t lane_offset,
                             uint64_t tick, hipStream_t st);

// Box.Sample() with per-element bounds (Box.cs:25-51,69-90): low / high device arrays of `dim` floats, out row-major [n][dim]
hipError_t launch_sample_box_elementwise(float *out, int64_t n, int32_t dim, const float *low, const float *high, uint64_t seed,
                                         uint64_t lane_offset, uint64_t tick, hipStream_t st);

}  // namespace gymnet
