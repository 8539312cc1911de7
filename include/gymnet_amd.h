/*
 * gymnet_amd.h — C ABI of the MI355X-native batched classic-control environment engine.
 *
 * This is the drop-in boundary for ONE path of SciSharp/Gym.NET: the per-instance
 * Env.Step()/Reset() hot path of the classic-control environments, replaced by one HIP kernel
 * launch over a structure-of-arrays batch held in HBM (one environment instance per GPU lane).
 * Plain C types only: no torch types, no C++ types, no callbacks.  A C# host binds it with
 * [DllImport("gymnet_amd")]; a C++ or ctypes host binds it the same way.
 *
 * Every entry point cites the reference interface it replaces, as path:line relative to the
 * Gym.NET source tree (/root/reference in the build container):
 *   IEnv / Env            src/Gym/Envs/IEnv.cs:11-22, src/Gym/Envs/Env.cs:13-41
 *   IVecEnv / VecEnv      src/Gym/Envs/IVecEnv.cs:8-19, src/Gym/Envs/VecEnv.cs:12-93
 *   VecEnvWrapper         src/Gym/Envs/VecEnvWrapper.cs:9-30
 *   CartPoleEnv           src/Gym.Environments/Envs/Classic/CartPoleEnv.cs:24-67,137-198
 *   Space/Box/Discrete    src/Gym/Spaces/{Space.cs:5-18,Box.cs:25-96,Discrete.cs:11-44}
 *   Step                  src/Gym/Observations/Step.cs:7-20
 *   errors                src/Gym/Exceptions/{InvalidActionError,AlreadySteppingError,NotSteppingError}.cs
 *
 * Conventions
 *   - Every function returns a gymnet_status (0 = ok, negative = error) unless documented
 *     otherwise; nothing throws or aborts across the ABI.  The message for the most recent
 *     failure on the calling thread is gymnet_last_error().
 *   - "host" pointers are ordinary CPU memory owned by the caller; "device" pointers (names
 *     starting with d_) are HIP device memory on the handle's device.  The library never keeps a
 *     caller pointer after the call returns, except: gymnet_vecenv_step_async keeps `actions`
 *     until it returns (it copies), and *_device calls use d_ pointers until the work queued on
 *     the handle's stream has run (gymnet_vecenv_sync).
 *   - Layouts.  Inside the engine everything is structure-of-arrays: state[state_dim][stride],
 *     obs[obs_dim][stride], reward[n], done[n].  At the HOST boundary observations are
 *     row-major [num_envs, obs_dim] float32 (what an NDArray of shape (N, D) holds), reward is
 *     float32[num_envs], done is uint8[num_envs] (0 / 1).
 *   - Dtypes: Discrete action int32; Box action float32; observation float32 (the DECLARED dtype
 *     of CartPoleEnv.ObservationSpace, CartPoleEnv.cs:48); reward float32 (Step.cs:9); done uint8.
 *     A handle created with GYMNET_FLAG_F64 (CartPole) computes in the reference's ACTUAL arithmetic:
 *     float64 state, and float64 observations at the boundary — what CartPoleEnv.Step really returns
 *     (CartPoleEnv.cs:166,185: the float64 state NDArray itself).  Every `obs` / `state` buffer of
 *     such a handle holds doubles; the parameters are typed void* for that reason.
 *   - A handle is single-caller-at-a-time (like an Env instance, which has no re-entrancy guard);
 *     different handles may be used from different threads.  All work of a handle is ordered on
 *     one HIP stream.
 */
#ifndef GYMNET_AMD_H
#define GYMNET_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GYMNET_ABI_VERSION 6   /* 2: gymnet_config.d_ext_obs_alt, gymnet_device_view.{obs_buffer,d_obs_alt}, groups;
                                  3: gymnet_env_info.{traffic_bytes_per_step,state_row_in_obs}, per-element Box sampling, compact
                                     terminal observations, pinned host staging;
                                  4: GYMNET_FLAG_F64 (float64 CartPole: observation / state buffers typed by the handle,
                                     gymnet_device_view.state_dtype), GYMNET_FLAG_COMPACT_RECORDS_ONLY, gymnet_launch_policy +
                                     set / get, gymnet_vecenv_get_array / _set_array / _get_seed (checkpoint of every array);
                                  5: GYMNET_FLAG_F64 is a first-class mode — it combines with DONE_LIST / FINAL_OBS / DOUBLE_BUFFER /
                                     COMPACT_RECORDS_ONLY / d_ext_obs(_alt) and with groups; every parameter that carries observation
                                     values (gymnet_config.d_ext_obs*, terminal observations, group replicas and host batches) is
                                     typed void* = the handle's state scalar (binary layout of the calls unchanged).  A launch-policy
                                     value that would not take effect is rejected;
                                  6: ACTION STREAM v2 — no signature or struct changed, the VALUES every sampling entry point draws
                                     did (see "batched space sampling" below): one Philox4x32-10 call now serves the four consecutive
                                     global lanes of a group instead of one lane.  Reset draws, and therefore every result computed
                                     from caller-supplied actions, are bit-for-bit what ABI 5 produced */

typedef enum gymnet_status {
    GYMNET_OK = 0,
    GYMNET_ERR_INVALID_ARG = -1,     /* ArgumentException / ArgumentNullException (VecEnv.cs:49, CartPoleEnv.cs:57) */
    GYMNET_ERR_INVALID_ACTION = -2,  /* InvalidActionError (src/Gym/Exceptions/InvalidActionError.cs:7-10) */
    GYMNET_ERR_HIP = -3,             /* a HIP runtime call failed */
    GYMNET_ERR_OOM = -4,             /* device or host allocation failed */
    GYMNET_ERR_NO_DEVICE = -5,       /* no usable AMD GPU: the engine has NO CPU fallback */
    GYMNET_ERR_ALREADY_STEPPING = -6,/* AlreadySteppingError (src/Gym/Exceptions/AlreadySteppingError.cs:8-10) */
    GYMNET_ERR_NOT_STEPPING = -7,    /* NotSteppingError (src/Gym/Exceptions/NotSteppingError.cs:4-6) */
    GYMNET_ERR_UNSUPPORTED = -8,
    GYMNET_ERR_RCCL = -9             /* an RCCL call failed, or librccl could not be loaded (group gather mode RCCL) */
} gymnet_status;

typedef enum gymnet_env_id {
    GYMNET_ENV_CARTPOLE = 0,     /* CartPoleEnv.cs (the only classic env present in the reference) */
    GYMNET_ENV_PENDULUM = 1,     /* absent from the reference (README.md:69-76); upstream gym Pendulum-v1 */
    GYMNET_ENV_MOUNTAINCAR = 2,  /* absent from the reference; upstream gym MountainCar-v0 */
    GYMNET_ENV_ACROBOT = 3,      /* absent from the reference; upstream gym Acrobot-v1 */
    GYMNET_ENV_MOUNTAINCAR_CONTINUOUS = 4  /* absent from the reference; upstream gym MountainCarContinuous-v0 (ABI 6: an added value,
                                              compatible) */
} gymnet_env_id;

/* gymnet_config.flags */
#define GYMNET_FLAG_AUTORESET        0x01u /* fuse the caller's `if (done) Reset()` (README.md:36-40) into the step kernel */
#define GYMNET_FLAG_VALIDATE_ACTIONS 0x02u /* reject actions outside Discrete(n) (Discrete.cs:38-40) before stepping, like
                                              LunarLanderEnv.cs:604-607; default mirrors Release-build CartPole (CartPoleEnv.cs:139,146) */
#define GYMNET_FLAG_DONE_LIST        0x04u /* emit the compacted list of lanes that finished in the last step */
#define GYMNET_FLAG_EPISODE_STATS    0x08u /* per-lane episode return / length bookkeeping (BasePlaySession.cs:58-69) */
#define GYMNET_FLAG_FINAL_OBS        0x10u /* with AUTORESET: keep the terminal observation of lanes that finished */
#define GYMNET_FLAG_F64              0x40u /* ABI 4, CartPole only: the reference's own arithmetic — float64 structure-of-arrays state, the literal
                                              operation sequence of CartPoleEnv.cs:141-167 in binary64 (float32-valued constants widened at use),
                                              reset draws with 53 random bits, float64 observations at the boundary.  Reproduces the reference's
                                              episode lengths free-running (the float32 engine guarantees 1e-5 per teacher-forced step only).
                                              73 B per env-step instead of 41.  Since ABI 5 it combines with every other flag, with d_ext_obs(_alt)
                                              (buffers of doubles) and with groups: the same kernels, instantiated for double (step_kernels.hpp) */
#define GYMNET_FLAG_COMPACT_RECORDS_ONLY 0x80u /* ABI 4, with DONE_LIST: the step kernel writes the finished lanes' episode records / terminal
                                              observations ONLY as compact records (gymnet_vecenv_done_records); the dense per-lane views
                                              (gymnet_vecenv_episode_stats / _final_obs, gymnet_device_view.d_finished_*) are then brought up to
                                              date on demand, for the most recent step only.  Default (flag clear): the step kernel keeps the
                                              dense views current itself, whatever the caller reads or skips */
#define GYMNET_FLAG_RESIDENT         0x100u /* ABI 5, num_envs <= 64 (the single-instance usage shape, README.md:32-52 / Env.cs:13-41): the host-boundary
                                              step / reset calls (gymnet_vecenv_step, _step_broadcast, _reset, _reset_where(NULL)) are served by a RESIDENT
                                              single-wave kernel that polls a mailbox in page-locked, device-mapped host memory: no kernel launch and no
                                              stream synchronize per step (two PCIe crossings instead of ~25 us).  Results are bit-identical to the
                                              launch path.  The kernel leaves by itself after ~50 ms without a command and is restarted on demand; every
                                              other entry point first tells it to leave.  While it is resident it occupies the handle's stream: a
                                              device-wide synchronize issued elsewhere in the process waits for it (up to the idle timeout).  Not with
                                              DONE_LIST / FINAL_OBS / DOUBLE_BUFFER / d_ext_obs / a caller's stream (GYMNET_ERR_UNSUPPORTED) */
#define GYMNET_FLAG_DOUBLE_BUFFER    0x20u /* two observation buffers, written alternately: the step launched after buffer A was
                                              written reads A and writes B, so a consumer (an all-gather of A over xGMI, a policy
                                              reading A) may still be using A while the next step runs.  For envs whose observation
                                              IS the state (CartPole, MountainCar, MountainCarContinuous) the state ping-pongs with it.  Which buffer holds
                                              the latest observation: gymnet_device_view.obs_buffer / d_obs */

typedef struct gymnet_vecenv gymnet_vecenv;   /* opaque handle: one batch ("VectorEnv") on one GPU */

typedef struct gymnet_config {
    uint32_t struct_size;       /* = sizeof(gymnet_config) */
    int32_t  env_id;            /* gymnet_env_id */
    int64_t  num_envs;          /* lanes owned by this handle (this rank's shard) — VecEnv.NumberOfEnvironments */
    int64_t  lane_offset;       /* global id of this handle's lane 0; reset draws are keyed by GLOBAL lane id, so a
                                   batch sharded over G handles/GPUs gives the same results as one handle */
    int32_t  device;            /* HIP device ordinal */
    uint32_t flags;             /* GYMNET_FLAG_* */
    uint64_t seed;              /* Env.Seed(int) (CartPoleEnv.cs:196-198): Philox key */
    void    *stream;            /* hipStream_t to order all work on; NULL = the library creates its own */
    void    *d_ext_obs;         /* optional device buffer [obs_dim][ext_obs_stride] (float32; float64 with GYMNET_FLAG_F64) to keep
                                   observations in (e.g. this
                                   rank's slice of an all-gather buffer).  It is LIVE STATE STORAGE, not an output copy: for
                                   envs whose observation IS the state (CartPole, MountainCar, MountainCarContinuous) every row, and for the others
                                   the rows listed in gymnet_env_info.state_row_in_obs (Pendulum obs[2]; Acrobot obs[4], obs[5]),
                                   are read back by the next step.  A consumer must not modify them in place (normalise /
                                   clip into its own buffer).  The same holds for d_ext_obs_alt.  NULL = library allocates */
    int64_t  ext_obs_stride;    /* elements between component arrays of d_ext_obs (>= num_envs) */
    int32_t  max_episode_steps; /* EXTENSION (the reference has no time limit): >0 truncates episodes;
                                   requires GYMNET_FLAG_EPISODE_STATS; done byte gets bit 1 (value 2) for truncation */
    int32_t  reserved;
    void    *d_ext_obs_alt;     /* with GYMNET_FLAG_DOUBLE_BUFFER and d_ext_obs: the caller's SECOND observation buffer (same
                                   stride), e.g. this rank's slice of a second all-gather buffer.  NULL = library allocates */
} gymnet_config;

typedef struct gymnet_env_info {
    uint32_t struct_size;
    int32_t  env_id;
    char     name[32];               /* "CartPole-v1", ... */
    int32_t  state_dim;
    int32_t  obs_dim;
    int32_t  obs_aliases_state;      /* 1: the observation arrays ARE the state arrays */
    int32_t  action_is_box;          /* 0: Discrete(action_n) int32; 1: Box(action_low, action_high, (1,)) float32 */
    int32_t  action_n;
    float    action_low, action_high;
    float    obs_low[8], obs_high[8];/* ObservationSpace bounds (CartPoleEnv.cs:46-48) */
    float    reward_low, reward_high;
    int32_t  algorithmic_bytes_per_step; /* bytes one env-step must move (CartPole: 41) */
    int32_t  traffic_bytes_per_step;     /* ABI 3: bytes one env-step really moves: less than the algorithmic figure where a state
                                            component the observation repeats verbatim is stored once (Pendulum 33 of 37,
                                            Acrobot 57 of 65) */
    int32_t  state_row_in_obs[8];        /* ABI 3: state component k is held in row state_row_in_obs[k] of the OBSERVATION array
                                            (Pendulum theta_dot = obs[2]; Acrobot dtheta1, dtheta2 = obs[4], obs[5]); -1 = in its
                                            own row of the state array.  Only matters to readers of gymnet_device_view.d_state;
                                            gymnet_vecenv_get_state / _set_state assemble the full [state_dim][num_envs] array */
} gymnet_env_info;

/* Device-side view of a handle: zero-copy access for a GPU-resident policy / trainer. */
typedef struct gymnet_device_view {
    uint32_t struct_size;
    int32_t  state_dim, obs_dim, obs_aliases_state;
    int64_t  num_envs, state_stride, obs_stride;
    void    *d_state;          /* [state_dim][state_stride] of state_dtype; rows listed in gymnet_env_info.state_row_in_obs are NOT
                                  kept here (they are rows of d_obs) */
    void    *d_obs;            /* [obs_dim][obs_stride] of state_dtype (== d_state when obs_aliases_state) */
    float   *d_reward;         /* [num_envs] */
    uint8_t *d_done;           /* [num_envs] */
    int32_t *d_steps_beyond_done; /* CartPole without AUTORESET: CartPoleEnv.cs:41 per lane; else NULL */
    void    *d_final_obs;      /* [obs_dim][num_envs] of state_dtype, FINAL_OBS only */
    int32_t *d_done_list;      /* [num_envs] compact list, valid after gymnet_vecenv_done_lanes(_device); DONE_LIST only */
    float   *d_episode_return; int32_t *d_episode_length;     /* running, EPISODE_STATS only */
    float   *d_finished_return; int32_t *d_finished_length;   /* last finished episode per lane */
    void    *stream;           /* hipStream_t all of the handle's work is ordered on */
    int32_t  obs_buffer;       /* GYMNET_FLAG_DOUBLE_BUFFER: index (0 / 1) of the buffer d_obs points at = the latest observation */
    int32_t  state_dtype;      /* ABI 4: gymnet_dtype of d_state / d_obs — GYMNET_DTYPE_F32, or GYMNET_DTYPE_F64 for a GYMNET_FLAG_F64 handle */
    void    *d_obs_alt;        /* GYMNET_FLAG_DOUBLE_BUFFER: the other buffer = what the NEXT step will write; else NULL */
} gymnet_device_view;

typedef enum gymnet_dtype { GYMNET_DTYPE_F32 = 0, GYMNET_DTYPE_F64 = 1 } gymnet_dtype;

/* ABI 4.  The step kernel's launch configuration.  The library chooses one at create from the batch size and the
 * buffers' alignment; gymnet_vecenv_set_launch_policy overrides fields (every field: -1 = leave as it is).  All configurations
 * of an env compute bit-identical results — this is a performance knob for probes, A/B timing and tests that pin a kernel form,
 * set through the ABI so that a host process's ENVIRONMENT never changes which kernel the library runs. */
typedef struct gymnet_launch_policy {
    uint32_t struct_size;          /* = sizeof(gymnet_launch_policy) */
    int32_t  vec;                  /* lanes per thread on wide accesses: 1, 4 (dwordx4 rows; not Acrobot), 2 (Acrobot packed-FP32 form; F64 handles) */
    int32_t  block;                /* threads per workgroup: 64 / 128 / 256 */
    int32_t  nt;                   /* non-temporal stream mask: 0 none, 12 action + reward / done, 15 every stream */
    int32_t  sequential_lanes;     /* multi-lane kernels (lean variant): Acrobot with vec 1 — lanes per thread, 1 (one-shot kernel) .. 5;
                                      Acrobot / F64 handles with vec 2 — lane PAIRS per thread, 1 .. 4; num_envs a multiple of
                                      2 * sequential_lanes * 256, except F64 handles with auto-reset (any batch size; their
                                      multi-pair kernel draws the fused reset once per thread-group of pairs whatever reset_form
                                      says).  A value > 1 the launcher would not resolve to -> GYMNET_ERR_INVALID_ARG */
    int32_t  reset_form;           /* fused auto-reset: 0 per-thread drain loop, 1 wave-compacted (wide kernels of the envs whose
                                      observation is the state: CartPole in both state scalars — F64: two lanes per reset —,
                                      MountainCar); also selects the per-step reset of the fused rollout */
    int32_t  lds_pipe;             /* Acrobot: 1 = producer / consumer form of the multi-lane kernel (needs num_envs % 512 == 0) */
    int32_t  occupancy_lds_bytes;  /* unused dynamic LDS per workgroup, for the one purpose of capping occupancy in probes */
    int32_t  graph;                /* gymnet_vecenv_rollout_device: 0 eager launches, 1 hipGraph replay, -2 back to "by batch size" */
} gymnet_launch_policy;

typedef struct gymnet_counters {
    uint32_t struct_size;
    uint32_t reserved;
    uint64_t tick;               /* engine tick: number of step/reset launches since seed (Philox counter word) */
    uint64_t lane_steps;         /* total env-steps executed */
    uint64_t stepped_after_done; /* lane-steps taken on an already-done lane: the reference's console warning
                                    (CartPoleEnv.cs:176-179), counted instead of printed */
    int64_t  last_done_count;    /* lanes that finished in the last step (DONE_LIST), else -1 */
} gymnet_counters;

/* ---- library-level ------------------------------------------------------------------------ */
int         gymnet_abi_version(void);
const char *gymnet_status_string(int status);
const char *gymnet_last_error(void);                 /* thread-local message of the last failure */
int         gymnet_device_count(int *count);         /* GYMNET_ERR_NO_DEVICE (count = 0) without a GPU */
/* Space descriptors an env's ctor builds (CartPoleEnv.cs:43-52): ActionSpace, ObservationSpace bounds. */
int         gymnet_env_describe(int env_id, gymnet_env_info *out);

/* ---- lifecycle: new VecEnv(...) / Close() / Dispose() ------------------------------------- */
/* VecEnv ctor (VecEnv.cs:13-18) + N x CartPoleEnv ctor (CartPoleEnv.cs:43-52).  State is undefined until reset. */
int gymnet_vecenv_create(const gymnet_config *cfg, gymnet_vecenv **out);
/* VecEnv.Close() (VecEnvWrapper.cs:26-30) / Env.Dispose() (Env.cs:38-40). */
int gymnet_vecenv_destroy(gymnet_vecenv *h);
/* VecEnv.Seed(int) (VecEnv.cs:44-46) -> Env.Seed (CartPoleEnv.cs:196-198).  DEVIATION: the reference hands every
 * env the SAME seed (identical reset streams); here lane i draws from Philox(key = seed, counter = (global lane, tick)).
 * Also rewinds the engine tick to 0. */
int gymnet_vecenv_seed(gymnet_vecenv *h, uint64_t seed);
/* VecEnv.Seed(int[]) (VecEnv.cs:48-53): one seed per lane; count != num_envs -> GYMNET_ERR_INVALID_ARG
 * (the reference throws ArgumentException).  Lane i then draws from Philox(key = seeds[i], ...). */
int gymnet_vecenv_seed_lanes(gymnet_vecenv *h, const uint64_t *seeds, int64_t count);

/* ---- host-boundary path (what an NDArray-based caller uses) --------------------------------- */
/* VecEnv.Reset() (VecEnvWrapper.cs:18-20) -> N x CartPoleEnv.Reset() (CartPoleEnv.cs:63-67): steps_beyond_done = -1,
 * state ~ U(-0.05,0.05)^4.  obs_out: host [num_envs, obs_dim] or NULL — float32, or float64 for a GYMNET_FLAG_F64 handle (here
 * and in every call below that takes obs_out). */
int gymnet_vecenv_reset(gymnet_vecenv *h, void *obs_out);
/* The caller's `if (done) Reset()` (README.md:36-40), batched: resets exactly the lanes with mask[i] != 0;
 * mask == NULL resets the lanes whose last returned done flag is set.  obs_out as above (all lanes).
 * With GYMNET_FLAG_AUTORESET the step itself already re-drew every finished lane, so mask == NULL is a NO-OP that only
 * returns the current observations (it used to draw those lanes a second time); an explicit mask still resets. */
int gymnet_vecenv_reset_where(gymnet_vecenv *h, const uint8_t *mask, void *obs_out);
/* EXTENSION of IVecEnv.Step (per-lane actions): N x CartPoleEnv.Step (CartPoleEnv.cs:137-186).
 * actions: host int32[num_envs] (Discrete) or float32[num_envs] (Box).  Outputs may each be NULL.  Blocks until
 * the outputs are written. */
int gymnet_vecenv_step(gymnet_vecenv *h, const void *actions, void *obs_out, float *reward_out, uint8_t *done_out);
/* IVecEnv.Step(int action) (IVecEnv.cs:15, VecEnvWrapper.cs:22-24): ONE scalar action broadcast to all lanes. */
int gymnet_vecenv_step_broadcast(gymnet_vecenv *h, int32_t action, void *obs_out, float *reward_out, uint8_t *done_out);
/* VecEnv.StepAsync (VecEnv.cs:63-65) / Env.StepAsync (Env.cs:23-25): queue the step, return immediately.
 * A second call before gymnet_vecenv_step_wait -> GYMNET_ERR_ALREADY_STEPPING. */
int gymnet_vecenv_step_async(gymnet_vecenv *h, const void *actions);
/* step_wait(): block until the queued step finished and copy its results out.  Without a pending
 * gymnet_vecenv_step_async -> GYMNET_ERR_NOT_STEPPING. */
int gymnet_vecenv_step_wait(gymnet_vecenv *h, void *obs_out, float *reward_out, uint8_t *done_out);
/* ABI 3.  Library-owned HOST buffers for this path, for a caller that can keep its NDArrays over unmanaged memory: actions
 * (int32 / float32 [num_envs]), obs (float32 [num_envs, obs_dim]), reward (float32 [num_envs]), done (uint8 [num_envs]) —
 * page-locked and mapped into the device, valid until gymnet_vecenv_destroy, allocated on the first call.  When the pointers
 * handed to gymnet_vecenv_step / _reset / _reset_where / _step_wait / _read ARE these buffers, the call runs without staging:
 * the actions are DMA'd straight out of the pinned buffer and ONE kernel writes observations (row-major), rewards and done flags
 * across PCIe into the others (no device-side pack buffer, no per-array memcpy).  Ordinary caller-owned memory keeps working
 * (staged copies).  Any out pointer may be NULL. */
int gymnet_vecenv_host_buffers(gymnet_vecenv *h, void **actions, void **obs, float **reward, uint8_t **done);
/* Copy the results of the most recent step/reset again (Step record, Step.cs:8-10). */
int gymnet_vecenv_read(gymnet_vecenv *h, void *obs_out, float *reward_out, uint8_t *done_out);

/* ---- device-resident path (no PCIe on the hot path; everything stream-ordered, non-blocking) --
 * The stream contract of every gymnet_vecenv_*_device call, here and in the sections below (render, pixel stack, episode memory, actor,
 * episode bookkeeping, sampling): all of its work — kernels, memsets, graph replays — is queued on the handle's stream
 * (gymnet_config.stream, or the library's own), in call order, and the call returns without waiting for it.  Two exceptions, both on the
 * host side of the call.  On a GYMNET_FLAG_VALIDATE_ACTIONS handle the calls that read the caller's Discrete actions
 * (gymnet_vecenv_step_device, gymnet_vecenv_step_repeat_device, gymnet_vecenv_rollout_device) block: Discrete.Contains is answered by one
 * readback before any state changes.  And a call may block the FIRST time it needs storage the handle allocates on demand (the episode-record
 * segments of gymnet_vecenv_rollout_fused_ex_device and its kin, a graph of gymnet_vecenv_rollout_device that evicts an older one); at
 * steady state none does.
 * Handle calls must not be captured by the caller into a graph of its own (hipStreamBeginCapture, torch.cuda.graph): they keep host-side
 * counters (the tick, the buffer parity, the attachments' marks) that a replay would not advance.  gymnet_vecenv_rollout_device replays
 * graphs of its own.  The handle-less exports below (gymnet_sample_*_device, gymnet_gae_device, gymnet_rollout_inputs_device,
 * gymnet_push_obs_device) keep nothing and are capturable. */
int gymnet_vecenv_reset_device(gymnet_vecenv *h);
int gymnet_vecenv_reset_where_device(gymnet_vecenv *h, const uint8_t *d_mask);   /* NULL = own done flags */
/* One vector step = ONE kernel launch.  d_actions: device int32[num_envs] / float32[num_envs]. */
int gymnet_vecenv_step_device(gymnet_vecenv *h, const void *d_actions);
/* `steps` consecutive vector steps, one kernel launch each, replayed from a cached hipGraph: step t reads
 * d_actions + (t % ring) * action_stride elements.  (The caller's hot loop, README.md:34-47, without host hops.) */
int gymnet_vecenv_rollout_device(gymnet_vecenv *h, const void *d_actions, int64_t steps,
                                 int64_t action_stride, int64_t ring);
/* Device-side rollout buffers (the example's replay memory, batched: examples/ReinforcementLearning/
 * ReinforcementLearning/MemoryTypes/ReplayMemory.cs:25-67).  Any pointer may be NULL = do not record that stream. */
typedef struct gymnet_rollout_buffers {
    void    *d_obs;     /* [steps][obs_dim][num_envs]  observation AFTER step t (after auto-reset, like the step API); float32 —
                           float64 for a GYMNET_FLAG_F64 handle */
    float   *d_reward;  /* [steps][num_envs] */
    uint8_t *d_done;    /* [steps][num_envs] */
} gymnet_rollout_buffers;
/* The same `steps` vector steps as gymnet_vecenv_rollout_device — bit-identical state, reward, done — fused into ONE
 * kernel launch: every lane keeps its state in registers across the steps, so per env-step only the action is read and
 * (optionally, rec != NULL) the recorded streams are written.  For open-loop / pre-generated action sequences only: no
 * policy can look at step t's observation before step t+1 (the closed-loop form is gymnet_vecenv_rollout_fused_ex_device with
 * GYMNET_ACTIONS_ACTOR: the handle's actor chooses every step's action inside the kernel).  (Since ABI 5 also on bookkeeping handles: see
 * gymnet_vecenv_rollout_fused_ex_device below, of which this is the ring-actions, no-episode-records form.) */
int gymnet_vecenv_rollout_fused_device(gymnet_vecenv *h, const void *d_actions, int64_t steps, int64_t action_stride,
                                       int64_t ring, const gymnet_rollout_buffers *rec);
/* ABI 5.  The fused rollout with what its CONSUMER needs (examples/ReinforcementLearning/ReinforcementLearning/PlaySessions/
 * BasePlaySession.cs:58-69 accumulates the episode reward and keeps the best episodes, MemoryTypes/ReplayMemory.cs:53-67 stores
 * them; TrainingPlaySession.cs:46-52 draws an epsilon-greedy action per step) — still ONE kernel launch for `steps` vector steps:
 *   - on a bookkeeping handle (EPISODE_STATS / DONE_LIST / FINAL_OBS / per-lane seeds; gymnet_vecenv_rollout_fused_device accepts
 *     those too now) the running episode return / length live in registers for the whole rollout, max_episode_steps truncates,
 *     per-lane seeds key the reset draws, the dense last-finished-episode views stay current, and the done list / records of
 *     "the most recent step" describe the rollout's last step: the handle ends in exactly the state `steps` single steps leave;
 *   - every episode that ends during the rollout leaves a compact record (step index t, lane, return, length) in the caller's
 *     arrays (wave ballot + one atomic per wave inside the kernel, gathered afterwards; unordered);
 *   - the ACTIONS can be drawn inside the kernel — GYMNET_ACTIONS_SAMPLE: ActionSpace.Sample() per lane and step, exactly the
 *     values gymnet_vecenv_sample_actions_device(seed = action_seed, tick = action_tick0 + t) would write; GYMNET_ACTIONS_
 *     EPSILON_GREEDY: gymnet_vecenv_compose_actions_device over the ring as the policy's actions — so a random rollout reads no
 *     action ring at all (0 B instead of 4 B per env-step), and d_rec_actions records what was taken.
 * Results are bit-identical to `steps` x (sample / compose, then gymnet_vecenv_step_device).  Stream-ordered, non-blocking. */
/* gymnet_rollout_spec.record_flags.  By default a rollout that keeps episode records loses none below ep_capacity.  NO_OVERFLOW selects the
 * kernel variant without the overflow path (8 % faster with records): episodes of lanes that finish very UNEVENLY — a few waves producing
 * most of them — can then be dropped below ep_capacity (a per-shard limit of 2 * ceil(ep_capacity / 256) + 64 records; d_ep_count[1] > [0]
 * says so).  Evenly finishing batches, e.g. random rollouts, never notice the difference. */
#define GYMNET_RECORDS_NO_OVERFLOW 1
/* GYMNET_ACTIONS_ACTOR (additive in ABI 6): the handle's actor chooses step t's action as gymnet_vecenv_actor_act_device(epsilon,
 * action_seed, action_tick0 + t) would, from the history the kernel keeps current (d_actions is ignored): bit-identical to `steps` x
 * (actor_act_device, step_device, actor_push_device), the final history included.  Needs a configured actor whose history is current;
 * float32 handles (GYMNET_ERR_UNSUPPORTED for float64 handles).  On a Box-action handle (Pendulum, MountainCarContinuous) the actor is the
 * Box actor of gymnet_vecenv_actor_box_config, step t's action is what gymnet_vecenv_actor_box_act_device(epsilon, action_seed,
 * action_tick0 + t) writes, epsilon means that call's rule and d_rec_actions is float32 [T][N]; without a Box actor the call fails as it
 * does without any actor.  Every flag combination of the other sources is accepted; GYMNET_RECORDS_NO_OVERFLOW is accepted and served
 * by the variant with the overflow segment (nothing is dropped below ep_capacity). */
typedef enum gymnet_action_source { GYMNET_ACTIONS_RING = 0, GYMNET_ACTIONS_SAMPLE = 1, GYMNET_ACTIONS_EPSILON_GREEDY = 2,
                                    GYMNET_ACTIONS_ACTOR = 3 } gymnet_action_source;
typedef struct gymnet_rollout_spec {
    uint32_t struct_size;        /* = sizeof(gymnet_rollout_spec) */
    int32_t  action_source;      /* gymnet_action_source */
    const void *d_actions;       /* RING: the actions; EPSILON_GREEDY: the policy's actions; SAMPLE: ignored (may be NULL) */
    int64_t  steps;
    int64_t  action_stride;      /* step t reads d_actions + (t % ring) * action_stride elements */
    int64_t  ring;
    uint64_t action_seed;        /* SAMPLE / EPSILON_GREEDY: Philox action stream key ... */
    uint64_t action_tick0;       /* ... and tick of step 0 (step t draws with tick action_tick0 + t) */
    float    epsilon;            /* EPSILON_GREEDY: exploration probability, [0, 1] */
    int32_t  record_flags;       /* episode records: 0, or GYMNET_RECORDS_NO_OVERFLOW (ABI 5 called this field `reserved`: 0 = the default).
                                    Zero-initialise the spec: any other bit is refused with GYMNET_ERR_INVALID_ARG. */
    /* dense per-step recording (the members of gymnet_rollout_buffers); any pointer NULL = not recorded */
    void    *d_rec_obs;          /* [steps][obs_dim][num_envs] observation AFTER step t; float32 — float64 for a GYMNET_FLAG_F64 handle */
    float   *d_rec_reward;       /* [steps][num_envs] */
    uint8_t *d_rec_done;         /* [steps][num_envs] */
    void    *d_rec_actions;      /* [steps][num_envs] the actions TAKEN (int32 / float32), or NULL */
    /* compact records of the episodes that ended during the rollout (bookkeeping handles); all NULL = none wanted */
    int32_t *d_ep_step;          /* [ep_capacity] step index t inside this rollout */
    int32_t *d_ep_lane;          /* [ep_capacity] lane */
    float   *d_ep_return;        /* [ep_capacity] episode return  (EPISODE_STATS) */
    int32_t *d_ep_length;        /* [ep_capacity] episode length  (EPISODE_STATS) */
    int64_t  ep_capacity;        /* records the arrays hold; a random-action CartPole rollout ends ~0.045 x num_envs episodes per step */
    uint32_t *d_ep_count;        /* [2]: [0] records written, [1] episodes that ended.  [1] > [0] exactly when more episodes ended than
                                    ep_capacity: then ep_capacity records are kept (which ones is unspecified) and the rest are only
                                    counted.  (Inside the kernel the records live in 256 per-shard segments — a wave appends to segment
                                    (wave index mod 256) with one atomic per flush — of 2 * ceil(ep_capacity / 256) + 64 records each;
                                    what a shard cannot hold, e.g. when a few waves produce most of the episodes, spills to one shared
                                    overflow segment of ep_capacity records, so an uneven batch loses nothing — unless record_flags asks
                                    for GYMNET_RECORDS_NO_OVERFLOW, round 5's behaviour.) */
} gymnet_rollout_spec;
int gymnet_vecenv_rollout_fused_ex_device(gymnet_vecenv *h, const gymnet_rollout_spec *spec);
/* ---- Frame skip: a decision's action held for several env steps inside ONE launch (the reference's IGameConfiguration.SkippedFrames,
 * BasePlaySession.cs:37-56) ----------------------------------------------------------------------------------------------------------
 * `repeat` = k >= 0 skipped frames; R = k + 1 sub-steps per DECISION.  repeat must lie in [0, 255] (else GYMNET_ERR_INVALID_ARG).  For a
 * launch of T decisions that starts at engine tick tick0, decision d, sub-step r:
 *   - the sub-step's engine tick is tick0 + d * R + r; the launch advances the handle's tick by T * R;
 *   - the action of decision d is chosen once and held for its R sub-steps: ring slice d % ring, or with sampled / epsilon-greedy actions the
 *     draw at action tick action_tick0 + d;
 *   - every lane takes sub-step 0 exactly as the one-step call would at that tick — without GYMNET_FLAG_AUTORESET including the
 *     steps_beyond_done rule and the stepped-after-done counter of a lane that was already done: every lane is LIVE at sub-step 0;
 *   - a live lane advances as the one-step kernel does at that tick (physics, episode return += reward, episode length += 1, truncation at
 *     max_episode_steps: the episode length counts env steps, not decisions);
 *   - when a live lane's done byte comes out non-zero at sub-step r, that byte is the decision's done byte; the terminal observation, the
 *     finished-episode views, the done list and the records are written as the one-step kernel writes them (a compact record of the fused
 *     form carries the DECISION index d as its step index); with AUTORESET the lane is re-drawn with the reset draw of tick
 *     tick0 + d * R + r, the draw a single step at that tick makes; and the lane is IDLE for sub-steps r + 1 .. R - 1: no step, no reward,
 *     no change of episode length or state.  At the next decision it sits on the first observation of its new episode (the reference starts
 *     an episode with a decision) — without AUTORESET on its terminal state, steps_beyond_done as the one step left it;
 *   - the decision's reward is the float32 sum of the sub-step rewards taken, added in sub-step order STARTING FROM THE FIRST SUB-STEP'S
 *     REWARD ITSELF (not from 0.0f: a -0.0f reward survives, and repeat = 0 is bit-identical to the one-step call);
 *   - afterwards d_obs / d_reward / d_done hold the last decision's observation (post-reset where a reset happened), summed reward and
 *     done byte; the d_rec_* arrays of a spec are per decision: [T][...][num_envs];
 *   - gymnet_counters.lane_steps grows by T * R * num_envs: it counts SLOTS — which sub-steps found their lane idle is not known to the host.
 * float32 and float64 handles, every env, every flag combination the fused rollout accepts.  repeat = 0 gives, bit for bit, what
 * step_device / step / rollout_fused_ex_device give (the calls forward).
 *
 * step_repeat_device: ONE decision with d_actions [num_envs]; validates like step_device on a VALIDATE_ACTIONS handle.  step_repeat: the
 * host-boundary form — stages the actions, runs one decision, copies out like gymnet_vecenv_step (it is not served by the resident kernel:
 * a GYMNET_FLAG_RESIDENT handle leaves residency first).  rollout_repeat_device: the fused form over an existing spec, spec.steps = the
 * number of decisions T (T * R must fit an int32); RING, SAMPLE and EPSILON_GREEDY with every check of rollout_fused_ex_device;
 * GYMNET_ACTIONS_ACTOR with repeat > 0 is GYMNET_ERR_UNSUPPORTED (run the unfused loop: act, step_repeat_device, push).
 * One decision — of any repeat — counts as one step for the attachments below: a pixel-stack, memory or actor push is accepted after it. */
int gymnet_vecenv_step_repeat_device(gymnet_vecenv *h, const void *d_actions, int32_t repeat);
int gymnet_vecenv_step_repeat(gymnet_vecenv *h, const void *actions, int32_t repeat, void *obs_out, float *reward_out, uint8_t *done_out);
int gymnet_vecenv_rollout_repeat_device(gymnet_vecenv *h, const gymnet_rollout_spec *spec, int32_t repeat);
/* Pack the SoA observations into row-major [num_envs, obs_dim] on the device (the NDArray layout; float32, or float64 for a
 * GYMNET_FLAG_F64 handle). */
int gymnet_vecenv_pack_obs_device(gymnet_vecenv *h, void *d_obs_rowmajor);
int gymnet_vecenv_sync(gymnet_vecenv *h);
int gymnet_vecenv_device_view(gymnet_vecenv *h, gymnet_device_view *out);
/* The launch configuration the handle chose for its step kernel (DESIGN.md §4 launch policy): lanes per thread on wide
 * accesses (1 / 2 / 4), threads per workgroup, non-temporal stream mask (0 / 12 / 15), and lanes per thread of the multi-lane
 * kernel that loads all of a thread's lanes first and then computes / stores them one after another (Acrobot; 1 = the
 * one-shot kernel).  Any out pointer may be NULL. */
int gymnet_vecenv_launch_policy(gymnet_vecenv *h, int32_t *vec, int32_t *block, int32_t *nt, int32_t *sequential_lanes);
/* ABI 4.  Override / read back the whole launch configuration (struct above).  A value the handle cannot run (dwordx4 lanes on an
 * unaligned external buffer, Acrobot's forms on another env, ...) -> GYMNET_ERR_INVALID_ARG and nothing changes.  Drops the
 * handle's captured graphs.  Synchronizes the handle's stream. */
int gymnet_vecenv_set_launch_policy(gymnet_vecenv *h, const gymnet_launch_policy *policy);
int gymnet_vecenv_get_launch_policy(gymnet_vecenv *h, gymnet_launch_policy *out);
/* ABI 3.  The kernel instantiation the handle's NEXT step launch runs, as text — e.g. "step_kernel<CartPole,4,true,false,15,1>"
 * (env, lanes per thread, AUTORESET, EXTRAS, non-temporal mask, reset form) or "step_kernel_pipe<Acrobot,4,true,15>".  It is
 * printed by the same function the launcher dispatches on, so a profile, a bench line or a parity test can name what ran
 * without copying the launch policy.  Diagnostic only: the spelling is not a stable interface. */
int gymnet_vecenv_kernel_name(gymnet_vecenv *h, char *buf, int32_t capacity);

/* ---- state access: teacher-forced parity tests, checkpoint / resume -------------------------- */
/* host [state_dim][num_envs] (structure-of-arrays), float32 — float64 for a GYMNET_FLAG_F64 handle.
 * CartPole: x, x_dot, theta, theta_dot (CartPoleEnv.cs:141-144).
 * set_state checks nothing: it may put a lane outside the env's state bounds, or hand it NaN / inf.  The contract of the next step:
 *   - inside the bounds (Acrobot: |theta| <= pi, |dtheta1| <= 4 pi, |dtheta2| <= 9 pi) the step is the upstream algorithm's;
 *   - outside them it is that of the project's float32 CPU restatement (the tests' twin), bit for bit.  Acrobot wraps an angle by at most six
 *     subtractions of 2 pi (enough for |theta| <= 13 pi before the wrap; the state bounds reach 29.73 rad): a larger angle, +-inf or
 *     NaN keeps what six subtractions leave, where upstream's loop would run on — or never end;
 *   - NaN is handed on by every clamp (upstream's min(max())): a poisoned lane stays NaN, is never done and is never reset by
 *     GYMNET_FLAG_AUTORESET, until max_episode_steps truncates it or the caller resets it. */
int gymnet_vecenv_get_state(gymnet_vecenv *h, void *state_soa);
int gymnet_vecenv_set_state(gymnet_vecenv *h, const void *state_soa);
/* steps_beyond_done per lane (CartPoleEnv.cs:41); only for CartPole without AUTORESET, else GYMNET_ERR_UNSUPPORTED. */
int gymnet_vecenv_get_steps_beyond_done(gymnet_vecenv *h, int32_t *out);
int gymnet_vecenv_set_steps_beyond_done(gymnet_vecenv *h, const int32_t *in);
int gymnet_vecenv_get_tick(gymnet_vecenv *h, uint64_t *tick);
int gymnet_vecenv_set_tick(gymnet_vecenv *h, uint64_t tick);
int gymnet_vecenv_counters(gymnet_vecenv *h, gymnet_counters *out);
/* ABI 4.  Every per-lane array a handle keeps, by id — together with the state, the tick and the seed this is a COMPLETE
 * checkpoint of any configuration (get_state / set_state double as checkpoint / resume): running episode return /
 * length (which drive the max_episode_steps truncation), the reward / done flags of the last step (which reset_where(NULL)
 * consumes), steps_beyond_done, the dense finished-episode views, the per-lane Philox keys of VecEnv.Seed(int[]).
 * `bytes` must equal the array's size (num_envs x element size; FINAL_OBS: obs_dim x num_envs x 4 — x 8 for a float64 handle —, structure-of-arrays).
 * An array the handle's configuration does not have -> GYMNET_ERR_UNSUPPORTED.  Both calls block.
 * set(LANE_SEEDS) installs the keys WITHOUT rewinding the tick (gymnet_vecenv_seed_lanes rewinds it); set(DONE) also forgets the
 * compacted done list of the step before (it described other flags). */
typedef enum gymnet_array_id {
    GYMNET_ARRAY_REWARD = 0,             /* float32 [num_envs] */
    GYMNET_ARRAY_DONE = 1,               /* uint8   [num_envs]  (bit 0 terminated, bit 1 truncated) */
    GYMNET_ARRAY_STEPS_BEYOND_DONE = 2,  /* int32   [num_envs]  CartPole without AUTORESET (CartPoleEnv.cs:41) */
    GYMNET_ARRAY_EPISODE_RETURN = 3,     /* float32 [num_envs]  EPISODE_STATS: running */
    GYMNET_ARRAY_EPISODE_LENGTH = 4,     /* int32   [num_envs] */
    GYMNET_ARRAY_FINISHED_RETURN = 5,    /* float32 [num_envs]  EPISODE_STATS: last finished episode per lane */
    GYMNET_ARRAY_FINISHED_LENGTH = 6,    /* int32   [num_envs] */
    GYMNET_ARRAY_FINAL_OBS = 7,          /* float32 (float64: F64 handle) [obs_dim][num_envs]  FINAL_OBS */
    GYMNET_ARRAY_LANE_SEEDS = 8          /* uint64  [num_envs]  after gymnet_vecenv_seed_lanes with distinct seeds */
} gymnet_array_id;
int gymnet_vecenv_get_array(gymnet_vecenv *h, int32_t which, void *out, int64_t bytes);
int gymnet_vecenv_set_array(gymnet_vecenv *h, int32_t which, const void *in, int64_t bytes);
/* The Philox key in use (Env.Seed(int), CartPoleEnv.cs:196-198) and whether per-lane keys are active.  Either out may be NULL. */
int gymnet_vecenv_get_seed(gymnet_vecenv *h, uint64_t *seed, int32_t *per_lane);

/* ---- CartPole frames (CartPoleEnv.Render, CartPoleEnv.cs:69-135) ----------------------------------------------------------
 * Frames of lanes [first_lane, first_lane + count) rasterised from the CURRENT observation buffer (what gymnet_vecenv_get_state
 * returns at that point of the stream: after an auto-reset step a finished lane shows its reset state; with GYMNET_FLAG_DOUBLE_BUFFER
 * the buffer d_obs points at).  Lane k's frame starts at out + (k - first_lane) * lane_stride bytes (lane_stride >= the frame's size;
 * the bytes between frames are not written) and is out_h rows of out_w pixels, top row first: RGB8 = 3 bytes per pixel, GRAY8 = 1.
 * The canvas is the reference's: 600 x 400, y down; scale = 600f / (2.4f * 2) and polelen = scale * (2 * 0.5f) as C# floats;
 * cx = (float)((double)x * scale + 300.0) (x = state row 0), theta = state row 2 as float.  Painted in order, the last shape
 * containing a sample wins: background white (255, 255, 255); track black [0, 600) x [300, 301); cart black [cx - 25, cx + 25] x
 * [285, 315]; pole (204, 153, 102), the points whose u = dx cos(theta) + dy sin(theta) is in [-5, 5] and v = dy cos(theta) - dx sin(theta)
 * in [5 - polelen, 5], (dx, dy) relative to the pivot (cx, 295) — positive theta leans right; axle (204, 153, 102), the disc of
 * radius 5 about (cx, 295).  GRAY8 paints white 255, black 0, pole and axle 160 (BT.709 luma, rounded).
 * Output pixel (i, j) of a crop (crop_x, crop_y, crop_w, crop_h) of the canvas takes the 16 samples
 * xs = crop_x + (j + (a + 0.5) / 4) * crop_w / out_w, ys = crop_y + (i + (b + 0.5) / 4) * crop_h / out_h (a, b = 0..3) and is
 * (sum of the 16 sample values + 8) >> 4 per channel — a supersampled box filter, not ImageSharp's scanline antialiasing.
 * A lane whose x or theta is not finite shows what stays defined (background and track; the cart and axle for a finite x).
 * Rendering changes nothing: state, tick, counters and the Philox stream are untouched.
 * Errors (nothing written): GYMNET_ERR_UNSUPPORTED for an env other than CartPole; GYMNET_ERR_INVALID_ARG for a NULL out, an unknown
 * format, lanes outside [0, num_envs) or count < 1, a crop not inside the canvas or of size <= 0, out_w / out_h outside [1, 16384],
 * or a lane_stride below one frame. */
enum { GYMNET_PIXELS_RGB8 = 1, GYMNET_PIXELS_GRAY8 = 2 };
/* into device memory, ordered on the handle's stream (does not block) */
int gymnet_vecenv_render_device(gymnet_vecenv *h, void *d_out, int32_t format, int64_t first_lane, int64_t count,
                                int32_t crop_x, int32_t crop_y, int32_t crop_w, int32_t crop_h,
                                int32_t out_w, int32_t out_h, int64_t lane_stride);
/* the same into host memory, staged through a device buffer the handle owns (allocated on first use); blocks */
int gymnet_vecenv_render(gymnet_vecenv *h, void *out, int32_t format, int64_t first_lane, int64_t count,
                         int32_t crop_x, int32_t crop_y, int32_t crop_w, int32_t crop_h,
                         int32_t out_w, int32_t out_h, int64_t lane_stride);

/* ---- CartPole pixel frame stacks (the Images runner's frame queue, ReplayMemory.cs:38-54, and input, ImageDataBuilder.cs:10-18) --
 * The handle owns at most one stack of processed frames per lane, kept on the device.  Lane k's stack starts at base + k * lane_stride
 * bytes and has `depth` slots: slot 0 the oldest, slot depth - 1 the newest, slot s at + s * frame_bytes.  A slot is out_h rows of
 * out_w elements, top row first; frame_bytes = out_w * out_h * (1, or 4 for BINARY_F32).  With a packed stride (lane_stride = depth *
 * frame_bytes) the buffer is exactly [num_envs][depth][out_h][out_w]: NCHW with the frames as channels.  The reference's vertical
 * 40 x 40 composition of two 40 x 20 frames (oldest on top) is this layout with depth = 2, crop (200, 150, 200, 150), 40 x 20.
 * The FRAME of a lane is what gymnet_vecenv_render_device draws from the current observation buffer for the same crop and size (same
 * samples, same rounding; float32 and float64 handles alike), processed by the format:
 *   GYMNET_STACK_GRAY8       byte for byte the GYMNET_PIXELS_GRAY8 frame;
 *   GYMNET_STACK_BINARY8     1 where that GRAY8 value is below 255, else 0: 1 exactly when one of the pixel's 16 samples is not
 *                            background.  It stands in for the reference's invert -> greyscale -> `R > 0 ? 1 : 0` (Imager.cs); the
 *                            reference resizes with ImageSharp's bicubic filter, which is not reproduced, so edge pixels may differ;
 *   GYMNET_STACK_BINARY_F32  the same as 1.0f / 0.0f.
 * config: checks its arguments and allocates the stack (the span (num_envs - 1) * lane_stride + depth * frame_bytes); with d_ext != NULL
 *   it adopts that device buffer instead (the caller keeps it alive until the stack is replaced, released or the handle destroyed).
 *   lane_stride = 0 means packed.  Then every slot of every lane gets the lane's current frame.  Calling it again replaces the stack;
 *   depth = 0 releases it (the other arguments are then not looked at).  gymnet_vecenv_destroy frees a stack the handle allocated.
 * reset_device: every lane with d_mask[lane] != 0 (d_mask NULL: every lane) gets its current frame in every slot; the others are not
 *   touched.  Call it after gymnet_vecenv_reset(_device) / _reset_where(_device) with the same mask.
 * push_device: per lane, once per step.  A lane that RESTARTS gets its current frame in every slot (gym's FrameStack reset
 *   convention); any other lane's slots 0 .. depth-2 take the old slots 1 .. depth-1 and the newest slot takes the current frame.  A lane
 *   restarts when d_done[lane] != 0 (either done bit: a truncation by max_episode_steps counts).  With d_done == NULL a
 *   GYMNET_FLAG_AUTORESET handle reads its own done bytes of the most recent step (gymnet_device_view.d_done); a handle without
 *   AUTORESET restarts no lane (its caller resets explicitly, then calls reset_device).  After a fused rollout pass the last row of its
 *   recorded d_done.
 * config, reset_device and push_device are ordered on the handle's stream and do not block.  None of the five calls changes anything
 *   but the stack: state, observations, tick, counters, the Philox stream and the done bytes stay as they were.  The stack is not part
 *   of a checkpoint (gymnet_vecenv_get_state / _get_array): after a restore, call reset_device.
 * read: copies the stacks of lanes [first_lane, first_lane + count) to host memory, packed (count * depth * frame_bytes bytes), and
 *   blocks: for hosts without a device allocator.
 * view: the stack's device pointer and geometry (any out pointer may be NULL).
 * Errors (nothing written, the previous stack unchanged): GYMNET_ERR_UNSUPPORTED for config on an env other than CartPole;
 * GYMNET_ERR_INVALID_ARG for an unknown format (GYMNET_PIXELS_RGB8 included), depth outside [0, 64], the crop / size rules of
 * gymnet_vecenv_render_device, a lane_stride below depth * frame_bytes or a span that overflows, for BINARY_F32 a d_ext or lane_stride
 * that is not a multiple of 4, reset / push / view / read before a stack is configured, a NULL read destination, or read lanes outside
 * [0, num_envs) or count < 1; GYMNET_ERR_OOM when the stack cannot be allocated. */
enum { GYMNET_STACK_GRAY8 = 2, GYMNET_STACK_BINARY8 = 3, GYMNET_STACK_BINARY_F32 = 4 };
int gymnet_vecenv_pixel_stack_config(gymnet_vecenv *h, int32_t format, int32_t depth,
                                     int32_t crop_x, int32_t crop_y, int32_t crop_w, int32_t crop_h,
                                     int32_t out_w, int32_t out_h, void *d_ext, int64_t lane_stride);
int gymnet_vecenv_pixel_stack_reset_device(gymnet_vecenv *h, const uint8_t *d_mask);
int gymnet_vecenv_pixel_stack_push_device(gymnet_vecenv *h, const uint8_t *d_done);
int gymnet_vecenv_pixel_stack_view(gymnet_vecenv *h, void **d_stack, int64_t *lane_stride, int64_t *frame_bytes);
int gymnet_vecenv_pixel_stack_read(gymnet_vecenv *h, void *out, int64_t first_lane, int64_t count);

/* ---- episode memory (the trainer's ReplayMemory.Memorize / EndEpisode, MemoryTypes/ReplayMemory.cs:25-67, and DataBuilder.BuildDataset,
 * DataBuilders/DataBuilder.cs:25-55) ------------------------------------------------------------------------------------------------
 * The handle owns at most one episode memory, kept on the device.  K = capacity (episodes kept), L = max_length (steps an episode may
 * have to be kept), S = history (steps per dataset row).
 * Transitions: step p of a lane's open episode stores the observation BEFORE the step (o_p), the action taken (int32 for Discrete,
 *   float32 for Box; the 4 bytes of d_actions[lane]) and the float32 reward.  o_0 is the observation the episode started from: the
 *   current observation at config or memory reset, or the post-step observation after an auto-reset.
 * Episode end: a push ends a lane's episode when its done byte is non-zero (either bit: a max_episode_steps truncation counts).  On a
 *   GYMNET_FLAG_AUTORESET handle the same push opens the next episode from the post-step observation; without AUTORESET the lane stays
 *   closed (its pushes record nothing) until memory_reset_device opens it.  The return is the float32 sum of the rewards in step order:
 *   bit-identical to the EPISODE_STATS finished return when the handle keeps one (the memory does not need that flag).
 * Keeping the best K: an ended episode's key is (return, end_tick, lane), ordered lexicographically, where end_tick is the engine tick
 *   after the step that ended it.  After every push the kept set is the top K keys of (kept set + the episodes that ended in that push).
 *   That is the reference's rule applied to episodes in (tick, lane) order — add when fewer than K are kept or return >= the lowest kept,
 *   then drop the lowest — with a newer episode winning ties of return.  An episode longer than L is not kept, in part or whole: it is
 *   counted as too_long.
 *   The order of returns is the float32 order with +0 and -0 as ONE return; +inf, -inf and denormals are ordinary values.  An episode
 *   whose return is NaN (a NaN or inf - inf among its rewards) is never kept, whatever the pool holds at the time: it counts in `ended`
 *   and in neither `admitted` nor — unless it is longer than L, which goes by the length alone — `too_long`.  The pool, the lowest kept
 *   return and the listing therefore never hold a NaN, and ordinary episodes go on being admitted after one.
 *   Equal keys: ticks only grow on their own, but a caller can set the tick backwards or restore a checkpoint (the memory is not part
 *   of one) and replay, so two ended episodes can have the same (return, end_tick, lane).  The kept set is then the top-K MULTISET of
 *   keys, which is unique: a greater key is never dropped for an equal one.  Every kept entry appears exactly once in `episodes` and
 *   in the dataset.  Among equal keys an entry already kept stays ahead of one that arrives, and their order in `episodes` and in the
 *   dataset is their order in the pool (pool index), the same in both; which of several equal kept entries a later push evicts is
 *   not specified.
 * Dataset: the kept episodes in descending key order; from each the first floor(len * 2 / 3) steps (DataBuilder.cs:33); one row per
 *   step: x, the action, for Discrete the one-hot of the action (float32 [action_n]) and the reward.
 *   GYMNET_MEMORY_PARAMS: x = float32 [S * obs_dim] = o_{p-S+1} .. o_p, oldest first, indices below 0 clamped to o_0 (float64
 *     observations rounded to float32).
 *   GYMNET_STACK_GRAY8 / _BINARY8 / _BINARY_F32 (CartPole only): x = [S][out_h][out_w] bytes (floats for BINARY_F32): the frames a
 *     pixel stack of the same format, crop, size and depth S held when the action was chosen, re-rendered from the stored observations.
 * Memory: (L + 1) * num_envs * row + K * L * row bytes, row = obs_dim * (4, or 8 for GYMNET_FLAG_F64) + 8, plus about 40 bytes per lane
 *   and 60 per kept episode: 12.6 GB for 2^20 CartPole float32 lanes with L = 500.  config_rollout with rollout_chunk = C adds C - 1 more
 *   staging slots of num_envs * row bytes and (C - 1) * num_envs * 16 bytes of candidates: 0.63 GB more at 2^20 CartPole lanes, C = 16.
 * config: capacity 0 releases the memory (the other arguments are then not looked at); else K in [1, 65536], history in [1, 64],
 *   max_length in [1, 2^24] or 0 for the handle's max_episode_steps (which must then be > 0).  Replaces any memory the handle had,
 *   with an empty pool, and opens every lane from its current observation.
 * config_rollout: config, plus rollout_chunk = C in [1, 64]: the number of consecutive steps one pass of push_rollout_device handles (a
 *   staging ring of L + C slots instead of L + 1, C candidate segments).  C = 1 is config.  Every other call treats the two alike.
 * reset_device: lanes with d_mask[lane] != 0 (NULL: every lane) abandon their partial episode and open one from their current
 *   observation (call it after gymnet_vecenv_reset(_device) / _reset_where(_device)); clear_pool != 0 also empties the pool and zeroes
 *   the counters.
 * push_device: once after each single vector step; d_actions are the actions that step took (device, [num_envs] of 4 bytes), d_done
 *   NULL means the handle's own done bytes.  Refused unless exactly one vector step ran since the last config, memory reset or push
 *   (a missed push, a multi-step rollout, or a reset of the handle without a memory reset in between), and after gymnet_vecenv_seed /
 *   _seed_lanes, set_tick (whatever the value), set_state, per-lane keys through set_array or a restored checkpoint until a memory reset:
 *   the open episodes describe observations that are gone.  The same holds for push_rollout_device.
 * push_rollout_device: the `steps` recorded rows of ONE step launch, ingested as `steps` single pushes would have been.  Accepted only when
 *   exactly one step launch of `steps` decisions ran since the last config, memory reset or push: any fused rollout
 *   (gymnet_vecenv_rollout_fused_device / _fused_ex_device / _rollout_repeat_device, every action source), or a single step with steps = 1.
 *   The buffers are what that launch wrote: d_rec_obs [steps][obs_dim][num_envs] in the handle's scalar, d_rec_reward and d_rec_done
 *   [steps][num_envs]; step t's actions are the num_envs 4-byte words at d_actions + (t % ring) * action_stride elements, as in
 *   gymnet_rollout_spec — a ring rollout passes its own ring, a sampled, epsilon-greedy or actor rollout its d_rec_actions with
 *   action_stride = num_envs, ring = steps.  Afterwards every observable of the memory (stats, episodes, dataset_size, dataset_device in
 *   every format, and every later push, ingest, reset and dataset) is bit for bit what step + push_device, `steps` times, would have left.
 *   Row t's episodes end at engine tick tick_before + (t + 1) * R, R = the launch's ticks per decision (frame skip).  The steps go in
 *   rollout_chunk at a time, two launches per pass; a memory from the plain config ingests with C = 1.
 * stats: kept episodes, episodes ended, episodes admitted into the kept set, episodes too long (any pointer may be NULL).  Blocks.
 * episodes: the kept episodes in descending key order, at most `capacity` of them (any array may be NULL); *count = how many are kept.
 *   Blocks.
 * dataset_size: the rows a dataset build writes now.  Blocks.
 * dataset_device: writes rows [0, min(rows, capacity_rows)) of the dataset: d_x ([rows][S * obs_dim] float32, or [rows][S][out_h][out_w]
 *   elements; crop and size follow gymnet_vecenv_render_device and are not looked at for GYMNET_MEMORY_PARAMS), d_action [rows],
 *   d_onehot [rows][action_n], d_reward [rows]; any of them may be NULL.
 * Everything but stats, episodes and dataset_size is ordered on the handle's stream and does not block; none of the calls changes state,
 *   observations, tick, counters, the Philox stream or the done bytes.  The memory is not part of a checkpoint.
 * Errors (nothing written): GYMNET_ERR_INVALID_ARG for arguments outside the ranges above, calls before a memory is configured, a null
 *   d_actions or a refused push (push_rollout_device: any null pointer, steps < 1, ring < 1, action_stride < 0, or a step count that is
 *   not the one launch's since the last memory event), an unknown dataset format, a d_onehot on a Box env, a BINARY_F32 d_x that is not 4-byte aligned, a
 *   negative capacity; GYMNET_ERR_UNSUPPORTED for a pixel dataset on an env other than CartPole; GYMNET_ERR_OOM when the memory cannot
 *   be allocated (the previous memory stays). */
enum { GYMNET_MEMORY_PARAMS = 0 };
int gymnet_vecenv_memory_config(gymnet_vecenv *h, int32_t capacity, int32_t max_length, int32_t history);
int gymnet_vecenv_memory_config_rollout(gymnet_vecenv *h, int32_t capacity, int32_t max_length, int32_t history, int32_t rollout_chunk);
int gymnet_vecenv_memory_reset_device(gymnet_vecenv *h, const uint8_t *d_mask, int32_t clear_pool);
int gymnet_vecenv_memory_push_device(gymnet_vecenv *h, const void *d_actions, const uint8_t *d_done);
int gymnet_vecenv_memory_push_rollout_device(gymnet_vecenv *h, int64_t steps, const void *d_rec_obs, const void *d_actions,
                                             int64_t action_stride, int64_t ring, const float *d_rec_reward, const uint8_t *d_rec_done);
int gymnet_vecenv_memory_stats(gymnet_vecenv *h, int64_t *kept, int64_t *ended, int64_t *admitted, int64_t *too_long);
int gymnet_vecenv_memory_episodes(gymnet_vecenv *h, float *ret, int32_t *len, uint64_t *end_tick, int32_t *lane, int64_t capacity,
                                  int64_t *count);
int gymnet_vecenv_memory_dataset_size(gymnet_vecenv *h, int64_t *rows);
int gymnet_vecenv_memory_dataset_device(gymnet_vecenv *h, int32_t format, int32_t crop_x, int32_t crop_y, int32_t crop_w, int32_t crop_h,
                                        int32_t out_w, int32_t out_h, void *d_x, int32_t *d_action, float *d_onehot, float *d_reward,
                                        int64_t capacity_rows);

/* ---- the actor (the trainer's BasePlaySession.ComposeAction -> Trainer.Predict -> _network.Forward and IndexOf(Max()),
 * PlaySessions/BasePlaySession.cs:78-81, Trainer.cs:91-92, and TrainingPlaySession.ComposeAction's epsilon-greedy wrapper,
 * PlaySessions/TrainingPlaySession.cs:46-52) --------------------------------------------------------------------------------------
 * The handle owns at most one actor: a fully connected ReLU network given by the caller and kept on the device, and a per-lane history
 * of the last S observations.  Training stays with the caller; the engine evaluates the weights it is given.
 * Network: L = num_layers in [1, 4] linear layers, widths w_0 .. w_L (widths[L + 1]) with w_0 = S * obs_dim, w_L = action_n, every width
 *   in [1, 64], at most 8192 parameters.  weights: float32, layer after layer, W_l [w_{l+1}][w_l] row-major (torch's nn.Linear.weight;
 *   NeuralNetworkNET's fully connected weights must be handed over in this [out][in] layout) followed by b_l [w_{l+1}]; count = their
 *   number.  Neuron j of layer l: acc = b_l[j]; acc = fmaf(W_l[j][i], x[i], acc) for i = 0 .. w_l - 1 (one rounding per product,
 *   ascending i); hidden layers then take acc > 0 ? acc : +0.0f; the last layer's values are the logits.  The action is the first index
 *   of the largest logit (argmax, not IndexOf(Max()) of a softmax: they differ only where exp rounding ties two outputs).
 * Input: x = o_{p-S+1} .. o_p, oldest first, each observation's obs_dim values contiguous, o_p the lane's current observation, indices
 *   below the episode's first observation clamped to it (float64 observations rounded to float32): the GYMNET_MEMORY_PARAMS row of the
 *   same step.
 * History: config and reset_device (lanes with d_mask[lane] != 0; NULL: every lane) fill every slot with the current observation;
 *   push_device, once after each single vector step: a lane whose done byte is non-zero (either bit; d_done NULL = the handle's own)
 *   refills every slot with its post-step observation, every other lane appends it.  Kept as float32 [S][obs_dim][lane_stride], a ring:
 *   view's *slot is the ring position of the newest observation, input row s (oldest first) is ring slot (slot + 1 + s) % S.
 * act_device: d_actions [num_envs] int32 = exactly what gymnet_vecenv_compose_actions_device(greedy, epsilon, d_actions, seed, tick)
 *   writes over the greedy actions (epsilon = 0: TestingPlaySession; > 0: TrainingPlaySession); d_logits [num_envs][action_n] or NULL.
 * load_device: count floats of device weights in the config layout replace the weights, ordered on the stream; the history is kept.
 * Staleness (GYMNET_ERR_INVALID_ARG, nothing written): act unless the history is current — no vector step since the last config,
 *   reset, push or actor rollout; push unless exactly one vector step ran since then.  A fused rollout with GYMNET_ACTIONS_ACTOR leaves
 *   the history current; any other rollout leaves it stale until an actor reset.  Every call that changes observations, Philox keys or
 *   the engine tick without being the one vector step a push expects — a reset of the handle that launches (gymnet_vecenv_reset(_device),
 *   _reset_where(_device); not the documented no-op of _reset_where with a NULL mask on an AUTORESET handle), gymnet_vecenv_seed /
 *   _seed_lanes, set_tick (whatever the value), set_state, per-lane keys through set_array, restoring a checkpoint — also leaves the
 *   history stale: call actor_reset_device after it.  act, push, value, boot and the actor rollout are refused after any of them, also
 *   where tick and step-launch count read as before (seed then reset; set_tick back to the old value): the handle counts these calls.
 *   gymnet_vecenv_set_array of any other array (reward, done, the episode arrays, terminal observations, steps_beyond_done) does NOT
 *   leave the history or the memory stale: a caller who rewrites the done bytes or the reward between a step and its push or boot gets
 *   the push or boot of what it wrote.
 *   So without AUTORESET the order is step, push, masked reset of the handle, actor_reset_device(mask).  On a GYMNET_FLAG_RESIDENT handle the host-boundary steps the resident kernel serves advance the tick
 *   but are not step launches, so a push after them is refused: drive an actor there with gymnet_vecenv_step_device (or the fused
 *   actor rollout).
 * Envs: Discrete-action envs (CartPole, MountainCar, Acrobot) on float32 handles, and float64 CartPole handles for config / reset /
 *   push / act; Box-action envs: GYMNET_ERR_UNSUPPORTED from actor_config (their actor is gymnet_vecenv_actor_box_config, below; load,
 *   reset, push and view serve both kinds).  num_layers 0 releases the actor (the other arguments are not looked at).
 *   Every call but config is ordered on the handle's stream and does not block; none changes state, observations, tick, counters or
 *   the done bytes.  The actor is not part of a checkpoint.
 * Errors (nothing written): GYMNET_ERR_INVALID_ARG for widths, count, history or epsilon outside the ranges above, null pointers, calls
 *   before an actor is configured and the staleness rules; GYMNET_ERR_UNSUPPORTED for Box-action envs; GYMNET_ERR_OOM. */
int gymnet_vecenv_actor_config(gymnet_vecenv *h, int32_t history, int32_t num_layers, const int32_t *widths, const float *weights,
                               int64_t count);
int gymnet_vecenv_actor_load_device(gymnet_vecenv *h, const float *d_weights, int64_t count);
int gymnet_vecenv_actor_reset_device(gymnet_vecenv *h, const uint8_t *d_mask);
int gymnet_vecenv_actor_push_device(gymnet_vecenv *h, const uint8_t *d_done);
int gymnet_vecenv_actor_act_device(gymnet_vecenv *h, int32_t *d_actions, float *d_logits, float epsilon, uint64_t seed, uint64_t tick);
int gymnet_vecenv_actor_view(gymnet_vecenv *h, float **d_history, int64_t *lane_stride, int32_t *slot);
/* A snapshot of the history on the device (an added export: the ABI version stays 6): d_out float32 [S][obs_dim][out_stride], unrolled —
 * row s = 0 is the oldest observation, ring slot (slot + 1 + s) % S of actor_view —, lane i in column i; columns [num_envs, out_stride) are
 * not touched.  One kernel on the handle's stream, non-blocking: unlike the ring actor_view hands out, the copy is the caller's and a later
 * push or actor rollout does not overwrite it.  Taken before a fused actor rollout it is the d_history0 of gymnet_rollout_inputs_device.
 * Serves Discrete and Box actors and float64 handles (the history is float32 everywhere).  GYMNET_ERR_INVALID_ARG, nothing written, where
 * actor_value_device is refused for the same reason — no actor configured, a stale history, a NULL or not 4-byte aligned pointer — and
 * for out_stride < num_envs.  No critic is needed.  Changes no state, no staleness mark and no tick. */
int gymnet_vecenv_actor_history_device(gymnet_vecenv *h, float *d_out, int64_t out_stride);
/* A Discrete actor's exploration setting (additive in ABI 6): (explore, temperature), read by act_device and by the fused rollout with
 * GYMNET_ACTIONS_ACTOR, which stays bit-identical to steps x (act_device, step_device, actor_push_device) under every setting.
 * The coin is unchanged — a lane explores if and only if word B of the aux stream is <= coin_threshold(epsilon) — and a lane that does
 * not explore takes the greedy action (argmax).  What an exploring lane takes:
 *   UNIFORM (default): ActionSpace.Sample() = umulhi(word A of the action stream, action_n), the behaviour described above, through the
 *   same kernels, whatever the temperature.
 *   SOFTMAX: a draw from softmax(logits / temperature), so at epsilon = 1 every lane samples the stochastic policy and at epsilon = 0
 *   nothing changes.  The draw is specified in float32, every operation rounded on its own, in this order (A = action_n <= 8, l_k the
 *   logits):
 *     1. m = the greedy logit (the value the argmax settles on).
 *     2. inv_tau = 1.0f / temperature, computed once on the host in float32.
 *     3. e_k = exp_neg((l_k - m) * inv_tau) for ascending k — a difference, a product, then exp_neg: t = a * 1.44269504f; a t that is
 *        not >= -125 (also a NaN) gives exactly +0.0f; otherwise n = rintf(t), f = t - n, p = the Horner chain of fmaf
 *        ((((((c7 f + c6) f + c5) f + c4) f + c3) f + c2) f + c1) f + 1 with c_i = float32(ln2^i / i!), and the result is p with n added
 *        to its exponent field as integer bits (csrc/exp_neg.hpp; not the device library's expf, whose bits a CPU cannot reproduce).
 *     4. c_k = c_{k-1} + e_k in index order (c_{-1} = 0), S = c_{A-1}.
 *     5. u = u01_24(word A), the lane's word of the action stream at (seed, global lane, tick) — the word UNIFORM feeds to umulhi.  (Word
 *        B is not u: on an exploring lane it is small by construction.)
 *     6. thr = u * S.
 *     7. The action is the first k with thr < c_k; if there is none (thr rounded up to S, S = 0, NaN or infinite logits) it is the greedy
 *        action.  So a chosen action has e_k > 0 or is the greedy one: an action whose weight underflowed to zero is never taken.
 *   Word A is drawn only when some lane of the wave explores, as under UNIFORM.
 * set_exploration: stored on the actor and read at the next act / actor rollout launch, so ordered on the handle's stream like the other
 *   actor calls; changes no history and no staleness state.  temperature is stored whatever explore is.  actor_config leaves the setting
 *   at (UNIFORM, 1.0) — also a re-config; load_device, push_device and reset_device keep it.  GYMNET_ERR_INVALID_ARG, nothing changed:
 *   no actor, a Box actor, an unknown enum value, a temperature that is not finite, is <= 0, or is so small that 1.0f / temperature is
 *   not finite.
 * get_exploration: any out pointer may be NULL; the same refusals for a handle without a Discrete actor (outputs untouched).
 * The log-probability of the action taken is recorded by gymnet_vecenv_actor_act_logp_device and
 *   gymnet_vecenv_rollout_fused_logp_device (below).  Out of scope: recording logits inside the fused rollout (re-evaluate the recorded
 *   inputs; for one step act_device's d_logits are the exact logits), a softmax for gymnet_vecenv_compose_actions_device, and the Box
 *   actor, whose policy is below. */
typedef enum gymnet_actor_explore { GYMNET_ACTOR_EXPLORE_UNIFORM = 0, GYMNET_ACTOR_EXPLORE_SOFTMAX = 1 } gymnet_actor_explore;
int gymnet_vecenv_actor_set_exploration(gymnet_vecenv *h, int32_t explore, float temperature);
int gymnet_vecenv_actor_get_exploration(gymnet_vecenv *h, int32_t *explore, float *temperature);
/* A Discrete actor's log-probability of the action taken (additive in ABI 6), for one act call and inside the fused rollout.
 * The quantity is specified in float32, every operation rounded on its own, like the softmax draw.  For a lane with logits l_0 .. l_{A-1}
 * (A = action_n <= 8), the actor's stored inv_tau = 1.0f / temperature, and the action j the lane takes, however it was chosen (greedy,
 * uniform exploration or softmax exploration):
 *   1. m = the greedy logit, the value the argmax settles on (step 1 of the draw).
 *   2. a_k = (l_k - m) * inv_tau, e_k = exp_neg(a_k), S = (((e_0 + e_1) + ...) + e_{A-1}) in index order: steps 3-4 of the draw, the same
 *      values (a wave that also runs the softmax draw computes them once).
 *   3. If !(S >= 1.0f), logp is the canonical quiet NaN 0x7FC00000, written as those bits: an infinite or NaN greedy logit, where every
 *      weight is +0.  With a finite m the greedy term is exactly 1.0f, so S lies in [1, 8].
 *   4. Otherwise L = log_pos(S) (csrc/log_pos.hpp; not the device library's logf, whose bits a CPU cannot reproduce): i = bits(S) +
 *      (0x3f800000 - 0x3f3504f3) as integers; k = float((i >> 23) - 127); f = float_of_bits((i & 0x007fffff) + 0x3f3504f3) - 1.0f;
 *      z = f * f; p = the Horner chain of fmaf (((((((p0 f + p1) f + p2) f + p3) f + p4) f + p5) f + p6) f + p7) f + p8 with the Cephes
 *      logf coefficients p0 = 7.0376836292e-2f .. p8 = 3.3333331174e-1f; r = fmaf(-0.5f, z, (f * z) * p); hi = k * 0.693359375f;
 *      s = hi + f; c = f - (s - hi); L = s + (fmaf(k, -2.12194440e-4f, r) + c).  Over every float32 in [1, 8]: log_pos(1.0f) = +0.0f, no
 *      result below +0, non-decreasing, within 1.20e-7 of the float64 log.
 *   5. logp = a_j - L, one subtraction, a_j selected by compares over the A values (never an indexed load).  A NaN result is stored as
 *      0x7FC00000 (possible only when uniform exploration takes an action whose own logit is NaN); -inf is stored as it comes.
 * The stored temperature is used whatever explore is (set_exploration stores it whatever explore is).  Under the default (UNIFORM, 1.0)
 *   logp is log softmax(logits)[j]; under (SOFTMAX, t) at epsilon = 1 it is exactly the behaviour policy's log-probability; for
 *   0 < epsilon < 1 it is the policy's log-probability of the action, NOT the epsilon-mixture's.  Against the float64 log-softmax of the
 *   same float32 logits at the true temperature the error is within 2^-20 * max(1, |logp|) (tests/test_actor_logp_host.py).
 * act_logp_device: with d_logp == NULL it IS gymnet_vecenv_actor_act_device (the call forwards; the same kernels run).  Otherwise
 *   d_actions and d_logits are bit for bit what act_device writes under the handle's setting, and d_logp [num_envs] is the quantity above
 *   (4-byte aligned).  The same staleness rules and refusals as act_device, nothing written on a refusal; a Box actor gives
 *   GYMNET_ERR_INVALID_ARG.  Served on float64 CartPole handles, as act_device is.  A request for logp runs kernels of their own
 *   (csrc/actor_logp.hip) under either setting.
 * rollout_fused_logp_device: with d_rec_logp == NULL it IS gymnet_vecenv_rollout_fused_ex_device(h, spec).  Otherwise
 *   spec->action_source must be GYMNET_ACTIONS_ACTOR and the handle's actor Discrete (else GYMNET_ERR_INVALID_ARG, nothing launched),
 *   every check of rollout_fused_ex_device applies, everything that call leaves for the spec is left bit for bit (state, observations,
 *   done bytes, tick, history, bookkeeping, every d_rec_* array, episode records and counters), and in addition
 *   d_rec_logp[t * num_envs + lane] is what act_logp_device(epsilon, action_seed, action_tick0 + t) writes at step t: the call is
 *   bit-identical to steps x (act_logp_device, step_device, actor_push_device).  d_rec_logp needs 4-byte alignment only; steps == 0
 *   writes nothing.
 * Out of scope: recording logits or an entropy, carrying logp through the episode memory.  (The Box actor's log-density has calls of its
 *   own: gymnet_vecenv_actor_box_act_logd_device, below.) */
int gymnet_vecenv_actor_act_logp_device(gymnet_vecenv *h, int32_t *d_actions, float *d_logits, float *d_logp, float epsilon, uint64_t seed,
                                        uint64_t tick);
int gymnet_vecenv_rollout_fused_logp_device(gymnet_vecenv *h, const gymnet_rollout_spec *spec, float *d_rec_logp);
/* The critic (additive in ABI 6): a second fully connected ReLU network attached to a configured actor, Discrete or Box, whose one output
 * is the lane's value estimate, for one call and inside the fused rollout.  Training stays with the caller.
 * Network: the actor's packed layout and limits — L in [1, 4] layers, every width in [1, 64], at most 8192 parameters, torch's nn.Linear
 *   layout, ReLU between the layers — with w_0 = the actor's input width S * obs_dim and w_L = 1; depth and hidden widths are the
 *   critic's own.
 * Value: the same fmaf chain in the same ascending input order that gives the actor its logits (gymnet_vecenv_actor_config, above), over
 *   the same input x = o_{p-S+1} .. o_p, taking the last layer's one value.  No new arithmetic: tests/_actor_twin.py's forward reproduces
 *   it bit for bit up to the sign of a zero.  value[t] is the value of the input step t's action is chosen from: the convention
 *   gymnet_gae_device documents for d_value.
 * actor_critic_config: host weights in actor_config's layout; needs a configured actor.  GYMNET_ERR_INVALID_ARG, nothing changed (a
 *   critic configured before stays): no actor, num_layers outside [0, 4], null pointers, a width outside [1, 64], widths[0] != S * obs_dim,
 *   widths[L] != 1, more than 8192 parameters, count != the parameters of these widths; GYMNET_ERR_OOM likewise.  num_layers == 0 removes
 *   the critic (the other arguments are not looked at).  Blocks until the weights are on the device, like actor_config.  A new
 *   actor_config or actor_box_config drops the critic — also a re-config, also num_layers 0 there; actor_load_device, actor_push_device,
 *   actor_reset_device, actor_set_exploration and actor_box_set_policy keep it.  The critic changes no history and no staleness state.
 * actor_critic_load_device: count floats of device weights of the configured shape replace the critic's, ordered on the handle's stream:
 *   the twin of actor_load_device.  GYMNET_ERR_INVALID_ARG: no actor, no critic, a null pointer, another count.
 * actor_value_device: d_value [num_envs] float32 = the critic over the current history, one kernel, ordered on the stream.  Serves every
 *   handle an actor serves, Box actors and float64 CartPole handles included.  The staleness rule of act_device.  GYMNET_ERR_INVALID_ARG,
 *   nothing written: no actor, no critic, a null or not 4-byte aligned pointer, a stale history.  This is the call that gives the last
 *   value after a rollout.
 * actor_act_value_device: with d_value == NULL it IS gymnet_vecenv_actor_act_logp_device (the call forwards).  Otherwise d_actions,
 *   d_logits and d_logp (which may be NULL) are bit for bit what that call writes, and d_value is what actor_value_device writes: the same
 *   act launch, then the value kernel behind it on the stream.  Discrete actors only (a Box actor: GYMNET_ERR_INVALID_ARG; call
 *   actor_box_act_device, then actor_value_device); every refusal of either call applies and nothing is written on a refusal.
 * rollout_fused_value_device: with d_rec_value == NULL it IS gymnet_vecenv_rollout_fused_logp_device(h, spec, d_rec_logp).  Otherwise
 *   spec->action_source must be GYMNET_ACTIONS_ACTOR, the handle's actor Discrete, and it must have a critic (else
 *   GYMNET_ERR_INVALID_ARG, nothing launched); every check of rollout_fused_ex_device applies; everything the logp call leaves is left bit
 *   for bit — d_rec_logp included, which may be NULL —, and in addition d_rec_value[t * num_envs + lane] is what actor_value_device would
 *   write before step t: the call is bit-identical to steps x (act_value_device, step_device, actor_push_device).  Both record pointers
 *   need 4-byte alignment only; steps == 0 writes nothing.  One kernel per form serves both exploration settings, with and without
 *   d_rec_logp (csrc/actor_value.hip).  A Box actor's values inside the fused rollout come from
 *   gymnet_vecenv_rollout_fused_box_logd_device (below).
 * Out of scope: a trunk shared between actor and critic; values carried through the episode memory; any gradient.  (V(terminal
 *   observation) for gymnet_gae_device's d_boot on time-limit rows: gymnet_vecenv_actor_boot_device and
 *   gymnet_vecenv_rollout_fused_value_boot_device, below.) */
int gymnet_vecenv_actor_critic_config(gymnet_vecenv *h, int32_t num_layers, const int32_t *widths, const float *weights, int64_t count);
int gymnet_vecenv_actor_critic_load_device(gymnet_vecenv *h, const float *d_weights, int64_t count);
int gymnet_vecenv_actor_value_device(gymnet_vecenv *h, float *d_value);
int gymnet_vecenv_actor_act_value_device(gymnet_vecenv *h, int32_t *d_actions, float *d_logits, float *d_logp, float *d_value, float epsilon,
                                         uint64_t seed, uint64_t tick);
int gymnet_vecenv_rollout_fused_value_device(gymnet_vecenv *h, const gymnet_rollout_spec *spec, float *d_rec_logp, float *d_rec_value);
/* The Box actor (additive in ABI 6): the same actor on a Box action space — Pendulum-v1 (obs_dim 3, bounds -2 .. 2) and
 * MountainCarContinuous-v0 (obs_dim 2, bounds -1 .. 1), float32 handles (neither env has a float64 mode).
 * Network: as above — L in [1, 4] layers, every width in [1, 64], at most 8192 parameters, torch's nn.Linear layout, ReLU between the
 *   layers, the same fmaf chain in ascending input order — with w_0 = S * obs_dim <= 64 (so S <= 21 on Pendulum, <= 32 on
 *   MountainCarContinuous) and w_L = the action dimension = 1.  Call the one output `raw`.
 * Greedy action: raw clamped to the env's bounds in the form the envs themselves use, raw < low ? low : (raw > high ? high : raw), low and
 *   high from gymnet_env_info (action_low / action_high); a NaN passes through it, as it does through Pendulum's own clamp.
 * Exploration (TrainingPlaySession.ComposeAction, TrainingPlaySession.cs:46-52, carried over to a Box space): let b be word B of the
 *   aux stream for (seed, global lane, tick).  If b <= coin_threshold(epsilon) — u01_24(b) <= epsilon — the action is ActionSpace.Sample()
 *   = low + (high - low) * u01_24(word A of the action stream): the value gymnet_vecenv_sample_actions_device writes for the same
 *   (seed, lane, tick).  Otherwise it is the greedy action.
 *   That is the default policy; gymnet_vecenv_actor_box_set_policy (below) offers a tanh head and Gaussian noise around the greedy action.
 * Out of scope: action dimensions above 1.
 * box_config: the arguments and checks of actor_config, with widths[num_layers] == 1; GYMNET_ERR_UNSUPPORTED on a Discrete-action env;
 *   num_layers 0 releases the actor.  The handle still owns at most one actor of either kind: configuring one replaces the other
 *   (everything is allocated before the old actor is released).
 * box_act_device: d_actions [num_envs] float32; d_raw [num_envs] float32 or NULL receives the unclamped output (the counterpart of
 *   d_logits).  The epsilon, null-pointer and staleness checks of actor_act_device.  Each act call refuses the other kind of actor with
 *   GYMNET_ERR_INVALID_ARG (nothing written).
 * History, staleness, load_device, reset_device, push_device and view are the rules above, shared by both kinds. */
int gymnet_vecenv_actor_box_config(gymnet_vecenv *h, int32_t history, int32_t num_layers, const int32_t *widths, const float *weights,
                                   int64_t count);
int gymnet_vecenv_actor_box_act_device(gymnet_vecenv *h, float *d_actions, float *d_raw, float epsilon, uint64_t seed, uint64_t tick);
/* A Box actor's policy (additive in ABI 6): (head, explore, sigma), read by box_act_device and by the fused rollout with
 * GYMNET_ACTIONS_ACTOR, which stays bit-identical to steps x (box_act_device, step_device, actor_push_device) under every policy.
 * head:    CLAMP (default): greedy = raw < low ? low : (raw > high ? high : raw).  TANH: greedy = mid + half * tanh(raw) in float32,
 *   mid = 0.5f * (low + high), half = 0.5f * (high - low) (0 and 2 on Pendulum, 0 and 1 on MountainCarContinuous, exactly), the product
 *   and the sum rounded on their own.  A NaN passes either head.  d_raw receives raw, unchanged, whatever the head.
 * explore: the coin is unchanged — a lane explores if and only if word B of the aux stream is <= coin_threshold(epsilon).
 *   SAMPLE (default): an exploring lane takes ActionSpace.Sample() = low + (high - low) * u01_24(word A), whatever the head.
 *   GAUSSIAN: an exploring lane takes clamp(greedy + sigma * z, low, high), z = sqrt(-2 ln u1) * cos(2 pi u2), with
 *   u1 = ((A >> 8) + 1) * 2^-24 from the lane's word A of the action stream (the u1 of the Box sampler's unbounded regime) and
 *   u2 = u01_24(N), N the lane's word of the noise stream: word (L & 3) of Philox(key = seed ^ 0xA0761D6478BD642F, counter = (L >> 2,
 *   tick)) for global lane L, laid out like words A and B.  (Word B is not u2: on an exploring lane it is small by construction.)
 *   A lane that does not explore takes greedy.
 * Exact: raw, which lanes explore, the words, and under sigma == 0 the value (clamp(greedy + 0 * z) == greedy).  Toleranced against
 *   float64: z within 1e-5 (|z| <= 5.77); the tanh greedy within half * 5 * 2^-24 plus one spacing of float32(max(|low|, |high|)); a
 *   Gaussian action within that, plus sigma * 1e-5, plus one spacing of float32(|greedy| + sigma * |z|).
 * set_policy: stored on the actor and read at the next act / actor rollout launch, so ordered on the handle's stream like the other
 *   actor calls; changes no history and no staleness state.  sigma is stored whatever explore is.  box_config leaves the policy at
 *   (CLAMP, SAMPLE, 0) — also a re-config; load_device, push_device and reset_device keep it.  GYMNET_ERR_INVALID_ARG, nothing changed:
 *   no actor, a Discrete actor, an unknown enum value, sigma not finite or below 0.
 * get_policy: any out pointer may be NULL; the same refusals for a handle without a Box actor. */
typedef enum gymnet_box_head    { GYMNET_BOX_HEAD_CLAMP = 0,     GYMNET_BOX_HEAD_TANH = 1 }        gymnet_box_head;
typedef enum gymnet_box_explore { GYMNET_BOX_EXPLORE_SAMPLE = 0, GYMNET_BOX_EXPLORE_GAUSSIAN = 1 } gymnet_box_explore;
int gymnet_vecenv_actor_box_set_policy(gymnet_vecenv *h, int32_t head, int32_t explore, float sigma);
int gymnet_vecenv_actor_box_get_policy(gymnet_vecenv *h, int32_t *head, int32_t *explore, float *sigma);
/* A Box actor's log-density of the action taken, and the critic's value inside its fused rollout (additive in ABI 6).  A Box action has
 * a density, not a probability: the calls and arguments are named logd.  Under any policy (head, explore, sigma) with sigma > 0, with g
 * the greedy action after the head and a the float32 action the lane takes — what d_actions / d_rec_actions receive, after the clamp:
 *     inv_sigma = (float)(1.0 / (double)sigma)                              on the host, once per launch
 *     c         = (float)(-log((double)sigma) - 0.91893853320467274178)     on the host, once per launch: -ln sigma - ln(2 pi) / 2
 *     d    = (a - g) * inv_sigma        float32, each operation rounding on its own
 *     h    = -0.5f * d
 *     logd = fmaf(h, d, c)
 *   This is log N(a; g, sigma^2), the density of the unclamped Gaussian at the action taken; a caller reproduces it as
 *   Normal(g_new, sigma).log_prob(rec_actions).  tests/_actor_box_logd_twin.py restates the lines and reproduces the bits; against the
 *   float64 closed form of the same float32 inputs the error is within 2^-21 * max(1, d^2, |c|) (tests/test_actor_box_logd_host.py).
 *   - The noise is added after the head, so a TANH head needs no Jacobian term.
 *   - It is recorded for every lane at the stored sigma, whatever explore is and whatever the coin says, as the Discrete logp reports
 *     the policy's probability under (UNIFORM, temperature) too.  A lane that does not explore has a == g and gets exactly c.  Under
 *     SAMPLE it is the Gaussian policy's density at the uniformly drawn action.  It is exactly the behaviour policy's density only at
 *     epsilon = 1 under GAUSSIAN, away from the bounds.
 *   - Where the clamp bit, it is the density at the bound; the point mass there is ignored (the usual PPO treatment).
 *   - A NaN g gives a NaN; a d^2 that overflows gives -inf.
 *   - sigma == 0 (the fresh default) or a sigma so small that 1.0f / sigma is not finite: GYMNET_ERR_INVALID_ARG from the two calls
 *     below, nothing written.  set_policy still stores such a sigma: the check is made where logd is asked for.
 *   Actions and raw outputs are the same bits with and without the request (one function composes them for both,
 *   csrc/actor_box_compose.hpp).
 * actor_box_act_logd_device: with d_logd == NULL it IS gymnet_vecenv_actor_box_act_device (the call forwards).  Otherwise d_actions and
 *   d_raw are bit for bit what that call writes under the handle's policy and d_logd [num_envs] float32 (4-byte aligned) is the quantity
 *   above.  The checks of box_act_device, then d_logd's alignment and the sigma; a Discrete actor gives GYMNET_ERR_INVALID_ARG (its call
 *   is gymnet_vecenv_actor_act_logp_device).  A request for logd runs kernels of their own (csrc/actor_box_logd.hip) under every policy,
 *   the default (CLAMP, SAMPLE) with sigma > 0 included.  A single step's value stays gymnet_vecenv_actor_value_device.
 * rollout_fused_box_logd_device: with both pointers NULL it IS gymnet_vecenv_rollout_fused_ex_device(h, spec).  Otherwise it refuses with
 *   GYMNET_ERR_INVALID_ARG, nothing launched, in this order: an action_source other than GYMNET_ACTIONS_ACTOR, no actor, a Discrete
 *   actor, a bad sigma, d_rec_value without a critic, a d_rec_logd that is not 4-byte aligned, a d_rec_value that is not; then every check
 *   of rollout_fused_ex_device applies.  Everything that call leaves for the spec is left bit for bit, and in addition
 *   d_rec_logd[t * num_envs + lane] is what box_act_logd_device(epsilon, action_seed, action_tick0 + t) writes at step t and
 *   d_rec_value[t * num_envs + lane] what actor_value_device would write before step t: the call is bit-identical to steps x
 *   (box_act_logd_device, actor_value_device, step_device, actor_push_device).  Either pointer may be NULL: d_rec_value alone is served
 *   here (and only here: the Discrete calls' d_rec_logp / d_rec_value and d_logp keep refusing a Box actor).  steps == 0 writes nothing.
 *   One kernel per form serves every policy and either pointer.
 * Out of scope: the Discrete calls' names lifted for a Box actor; noise before the TANH head (a squashed Gaussian with its Jacobian);
 *   a learned or per-lane sigma; logd carried through the episode memory.  (V(terminal observation) for gymnet_gae_device's d_boot rows:
 *   gymnet_vecenv_rollout_fused_box_boot_device, below.) */
int gymnet_vecenv_actor_box_act_logd_device(gymnet_vecenv *h, float *d_actions, float *d_raw, float *d_logd, float epsilon, uint64_t seed,
                                            uint64_t tick);
int gymnet_vecenv_rollout_fused_box_logd_device(gymnet_vecenv *h, const gymnet_rollout_spec *spec, float *d_rec_logd, float *d_rec_value);
/* V(terminal observation) on time-limit rows (additive in ABI 6): the array gymnet_gae_device takes as d_boot, for one step and inside the
 * fused actor rollout, for a Discrete or a Box actor with a critic on a handle with max_episode_steps > 0.  For a lane with this step's
 * done byte d, history depth S, ring o_{p-S+1} .. o_p (the input the step's action was chosen from) and terminal observation o_term (the
 * post-step observation before any reset):
 *     boot = (d & 2) ? critic(o_{p-S+2}, .., o_p, (float)o_term)[0] : +0.0f
 *   The critic is the fmaf chain of actor_value_device over the input that call would read had o_term been pushed with a done byte of 0
 *   (S == 1: o_term alone).  No new arithmetic: tests/_actor_twin.py's forward reproduces it bit for bit up to the sign of a zero.
 *   d == 3 (terminated and truncated in the same step) gets the value too; gymnet_gae_device lets "terminated" win and ignores it.  A row
 *   without bit 1 gets +0.0f, never stale memory.
 * actor_boot_device: d_boot [num_envs] float32 (4-byte aligned), one kernel, ordered on the stream.  Call it after a vector step and
 *   before actor_push_device: it needs exactly the state a push needs — one vector step since the last actor config, reset or push, on
 *   the decision clock, so it also follows step_repeat_device — and reads the handle's done bytes and o_term from memory: on an AUTORESET
 *   handle the dense GYMNET_FLAG_FINAL_OBS rows, otherwise the handle's current observation (cast to float32 as actor_push_device casts:
 *   float64 handles are served).  It changes nothing else: not the history, not the staleness state, not the tick.
 *   GYMNET_ERR_INVALID_ARG, nothing written, in this order: no actor, no critic, a null or misaligned pointer, any other step count since
 *   the last push, max_episode_steps == 0 (nothing can be truncated), an AUTORESET handle without GYMNET_FLAG_FINAL_OBS, or with
 *   GYMNET_FLAG_COMPACT_RECORDS_ONLY + GYMNET_FLAG_DONE_LIST (the dense rows are not maintained then).
 * rollout_fused_value_boot_device: with d_rec_boot == NULL it IS gymnet_vecenv_rollout_fused_value_device(h, spec, d_rec_logp,
 *   d_rec_value).  rollout_fused_box_boot_device: with d_rec_boot == NULL it IS gymnet_vecenv_rollout_fused_box_logd_device(h, spec,
 *   d_rec_logd, d_rec_value).  Otherwise, for both: d_rec_boot without d_rec_value is GYMNET_ERR_INVALID_ARG; then every check and refusal
 *   text of the forwarding target applies in its order (so: a critic); then max_episode_steps == 0 and a d_rec_boot that is not 4-byte
 *   aligned are GYMNET_ERR_INVALID_ARG; then every check of rollout_fused_ex_device.  Nothing is launched on a refusal.  Everything the
 *   forwarding target leaves is left bit for bit, and in addition d_rec_boot[t * num_envs + lane] is what actor_boot_device would write
 *   after step t: the call is bit-identical to steps x (act_value_device / box_act_logd_device + actor_value_device, step_device,
 *   actor_boot_device, actor_push_device).  GYMNET_FLAG_FINAL_OBS is not needed: o_term is taken from the kernel's registers before the
 *   fused reset.  steps == 0 writes nothing.  A wave in which no lane is truncated skips the evaluation (csrc/actor_boot.hip).
 * Out of scope: boot carried through the episode memory's rows; the fused actor rollout's frame skip; any gradient. */
int gymnet_vecenv_actor_boot_device(gymnet_vecenv *h, float *d_boot);
int gymnet_vecenv_rollout_fused_value_boot_device(gymnet_vecenv *h, const gymnet_rollout_spec *spec, float *d_rec_logp, float *d_rec_value,
                                                  float *d_rec_boot);
int gymnet_vecenv_rollout_fused_box_boot_device(gymnet_vecenv *h, const gymnet_rollout_spec *spec, float *d_rec_logd, float *d_rec_value,
                                                float *d_rec_boot);

/* ---- episode bookkeeping (the step AFTER the path: BasePlaySession.cs:58-69) ------------------ */
/* Lanes that finished in the most recent step (unordered). Needs GYMNET_FLAG_DONE_LIST. */
int gymnet_vecenv_done_lanes(gymnet_vecenv *h, int32_t *lanes_out, int64_t capacity, int64_t *count);
/* Device-side form: writes the compact list to d_lanes_out (capacity num_envs int32; NULL = the handle's own buffer,
 * gymnet_device_view.d_done_list) and the count to *d_count_out.  Stream-ordered, does not block.  (Inside the step
 * kernel the list is built per wave with ballot + one atomic into one of 256 shard counters; this call gathers the
 * shards.) */
int gymnet_vecenv_done_lanes_device(gymnet_vecenv *h, int32_t *d_lanes_out, uint32_t *d_count_out);
/* ABI 3.  The RECORDS of the lanes that finished in the most recent step, compacted (unordered; all arrays in the same order):
 * lane ids, with EPISODE_STATS the finished episode's return and length, with FINAL_OBS its terminal observation as rows
 * [count][obs_dim] (float32; float64 for a GYMNET_FLAG_F64 handle — here and in gymnet_vecenv_final_obs) — what a trainer consumes per step (BasePlaySession.cs:58-69: accumulate reward, count steps per episode)
 * without shipping num_envs flags to the host.  Inside the step kernel every finished lane's record is written AT ITS POSITION
 * in the (sharded) done list, so a wave's ~11 finished lanes write a few contiguous cache lines instead of one scattered line
 * per lane and array.  Any out pointer may be NULL; at most `capacity` records are copied, *count is the true number.
 * Needs GYMNET_FLAG_DONE_LIST. */
int gymnet_vecenv_done_records(gymnet_vecenv *h, int32_t *lanes_out, float *return_out, int32_t *length_out, void *final_obs_out,
                               int64_t capacity, int64_t *count);
/* Device-side form (stream-ordered, does not block): caller-owned device arrays of `capacity` records each (d_final_obs:
 * [capacity][obs_dim] row-major); *d_count receives the true number.  Any array may be NULL. */
int gymnet_vecenv_done_records_device(gymnet_vecenv *h, int32_t *d_lanes, float *d_return, int32_t *d_length, void *d_final_obs,
                                      int64_t capacity, uint32_t *d_count);
/* DENSE views, one row per lane.  Last finished episode's return and length per lane (0 length = none finished yet); needs
 * EPISODE_STATS.  Terminal observations, host [num_envs, obs_dim], rows of lanes that never finished are 0; needs FINAL_OBS.
 * The step kernel maintains these arrays itself (scattered stores), so they are current after ANY sequence of steps, rollouts or
 * graph replays, read or not.  Only with GYMNET_FLAG_COMPACT_RECORDS_ONLY (an opt-in beside DONE_LIST) does the step write the
 * compact records alone; each call of these getters then first applies the records of the MOST RECENT step to the dense arrays,
 * and records of steps the caller did not read are not in the dense view (use gymnet_vecenv_done_records every step). */
int gymnet_vecenv_episode_stats(gymnet_vecenv *h, float *finished_return, int32_t *finished_length);
int gymnet_vecenv_final_obs(gymnet_vecenv *h, void *final_obs_out);

/* ---- batched space sampling (the step BEFORE the path: ActionSpace.Sample(), TrainingPlaySession.cs:46-49) -- */
/* All sampling below draws from the ACTION stream (version 2, ABI 6).  A sampled action consumes one 32-bit word and a
 * Philox4x32-10 call yields four, so the four consecutive GLOBAL lanes of a group share one call:
 *     word A of global lane L at tick t = word (L & 3) of Philox(key = seed ^ 0x9E3779B97F4A7C15, counter = (L >> 2, t))
 *     word B of global lane L at tick t = word (L & 3) of Philox(key = seed ^ 0xD6E8FEB86659FD93, counter = (L >> 2, t))
 * with L = lane_offset + i.  A is the ActionSpace.Sample() word; B is drawn only by the consumers that need a second word (the
 * epsilon-greedy coin, the second uniform of Box.cs:82's normal).  Neither key is the reset draws' (key = seed), so
 * ActionSpace.Sample() called with an env's own (seed, tick) never replays the words of that env's reset draws; values depend on
 * the GLOBAL lane only, so a sharded batch samples what the whole batch would (any lane_offset, aligned to a group or not).
 * (Version 1, ABI <= 5: a whole call per lane, counter (L, t), words 0 and 1.  The reference's own stream is NumSharp's
 * un-vendored generator — CartPoleEnv.cs:49, Discrete.cs:17-28 — and is pinned by nothing)
 * The four handle-less samplers run on `stream` (a hipStream_t of `device`; NULL = default): stream-ordered, non-blocking, capturable (no
 * allocation, copy or synchronise) — seed, lane_offset and tick are kernel arguments, so a captured call replays the same draw.
 * Discrete.Sample() without mask (Discrete.cs:17-28): start + randint(0, n).  Element i = start + hi32(word A * n). */
int gymnet_sample_discrete_device(int device, void *stream, int32_t *d_out, int64_t count, int32_t n, int32_t start,
                                  uint64_t seed, uint64_t lane_offset, uint64_t tick);
/* Discrete.Sample(mask) (Discrete.cs:18-26): valid = {k : mask[k] == 1}; none -> start, else start + valid[hi32(word A * |valid|)].
 * d_mask: device uint8, one row of n bytes per element (mask_stride = n) or ONE row shared by all elements (mask_stride = 0).
 * On `stream`: stream-ordered, non-blocking, capturable (no allocation, copy or synchronise). */
int gymnet_sample_discrete_masked_device(int device, void *stream, int32_t *d_out, int64_t count, int32_t n, int32_t start,
                                         const uint8_t *d_mask, int64_t mask_stride, uint64_t seed, uint64_t lane_offset, uint64_t tick);
/* Box.Sample() (Box.cs:69-90), the reference's four regimes per element: bounded -> uniform(low, high);
 * low only -> low + Exp(1); high only -> high + Exp(1) (sic, Box.cs:84); unbounded -> Normal(0.5, 1) (sic, Box.cs:82).
 * low = -INFINITY / high = +INFINITY select the regime.  The bounded draw is low + (high - low) * u in float32; where high - low
 * overflows float32 (bounds as wide as CartPole's +-float.MaxValue velocities) it is low * (1 - u) + high * u: finite, inside the bounds.
 * On `stream`: stream-ordered, non-blocking, capturable (no allocation, copy or synchronise). */
int gymnet_sample_box_device(int device, void *stream, float *d_out, int64_t count, float low, float high,
                             uint64_t seed, uint64_t lane_offset, uint64_t tick);
/* ABI 3.  Box.Sample() for a Box built from Low / High ARRAYS (Box.cs:25-51: `new Box(NDArray low, NDArray high)`), e.g. an
 * observation space whose velocity components are unbounded: `count` samples of `dim` elements each, row-major [count][dim];
 * d_low / d_high are device arrays of `dim` floats and every element picks ITS OWN regime from its own bounds, like the
 * reference's boolean masks (Box.cs:74-85).  gymnet_sample_box_device above is the scalar-bounds form (one pair for every
 * element: the four envs' action spaces); for dim = 1 both draw the same values.
 * On `stream`: stream-ordered, non-blocking, capturable (no allocation, copy or synchronise). */
int gymnet_sample_box_elementwise_device(int device, void *stream, float *d_out, int64_t count, int32_t dim, const float *d_low,
                                         const float *d_high, uint64_t seed, uint64_t lane_offset, uint64_t tick);
/* ActionSpace.Sample() for every lane of a handle into d_actions (int32 / float32 [num_envs]). */
int gymnet_vecenv_sample_actions_device(gymnet_vecenv *h, void *d_actions, uint64_t seed, uint64_t tick);
int gymnet_vecenv_sample_actions(gymnet_vecenv *h, void *actions_out, uint64_t seed, uint64_t tick);
/* ActionSpace.Sample(mask) for every lane of a handle (Discrete action spaces only; Box.Sample(mask) throws in the
 * reference, Box.cs:70 -> GYMNET_ERR_UNSUPPORTED). */
int gymnet_vecenv_sample_actions_masked_device(gymnet_vecenv *h, int32_t *d_actions, const uint8_t *d_mask, int64_t mask_stride,
                                               uint64_t seed, uint64_t tick);
/* The caller's epsilon-greedy composer, batched (examples/ReinforcementLearning/ReinforcementLearning/PlaySessions/
 * TrainingPlaySession.cs:46-52: `if (Random.NextDouble() <= _epsilon) return ActionSpace.Sample(); return policy action`).
 * Lane i: u = 24-bit uniform from word B of (seed, global lane, tick); out[i] = (u <= epsilon) ? the
 * Discrete.Sample() draw of gymnet_vecenv_sample_actions_device for the same (seed, tick) : d_policy_actions[i].
 * Discrete action spaces only. */
int gymnet_vecenv_compose_actions_device(gymnet_vecenv *h, const int32_t *d_policy_actions, float epsilon, int32_t *d_actions_out,
                                         uint64_t seed, uint64_t tick);

/* ---- advantages and returns over a recorded rollout (the target of an on-policy update) ------------------------------------
 * Generalized advantage estimation GAE(gamma, lambda) and advantage + value over the rows a fused rollout recorded (d_rec_reward,
 * d_rec_done), one kernel launch, handle-less like the samplers above: on `stream` (a hipStream_t of `device`; NULL = default),
 * stream-ordered, non-blocking, capturable (no allocation, copy or synchronise).  An added export: the ABI version stays 6.
 * Arrays are [steps][stride] rows with stride >= count; lane i is column i, columns [count, stride) are neither read nor written:
 *     r = d_reward[t][i] float32;  d = d_done[t][i] uint8 (bit 0 terminated, bit 1 truncated by max_episode_steps);
 *     v = d_value[t][i] float32: the value of the observation the action of step t was chosen from;
 *     d_last_value[i] float32: the value of the observation after step steps-1;  d_boot[t][i] float32 (optional, see below).
 * Relative to a rollout's d_rec_obs: v[0] is the value of the observation before the rollout, v[t] = V(rec_obs[t-1]) and
 * last_value = V(rec_obs[steps-1]).  With frame skip the rows are per DECISION and gamma discounts decisions; a discount that is
 * exact per env step under idle sub-steps is not built.
 * The arithmetic is float32, every operation rounds on its own, the only fusions are the two fmaf below; gl = gamma * lambda is one
 * float32 product formed once.  Per lane, for t = steps-1 .. 0, carrying A (start +0.0f) and vnext (start d_last_value[i], or +0.0f
 * where d_last_value is NULL):
 *     cut   = d != 0
 *     nv    = (d & 1) ? +0.0f : (d & 2) ? (d_boot ? d_boot[t][i] : +0.0f) : vnext          terminated wins over truncated
 *     delta = fmaf(gamma, nv, r) - v
 *     A     = cut ? delta : fmaf(gl, A, delta)
 *     d_advantage[t][i] = A;   d_return[t][i] = A + v;   vnext = v
 * d_value NULL: every v (and the vnext taken from it) is +0.0f; d_last_value and d_boot are still honoured if given (both are allowed
 * without d_value: no combination of the three is refused).  With lambda = 1 the advantage is then the discounted reward-to-go, the
 * REINFORCE target, and at gamma = 1 the episode return the reference trainer ranks by (BasePlaySession.cs:58-69).
 * d_boot carries V(terminal observation) for lanes a time limit truncated: under GYMNET_FLAG_AUTORESET rec_obs[t] already holds the new
 * episode's first observation there, so v[t+1] must not be used across a done row, and it is not.  Without d_boot a truncation is
 * treated as a termination.
 * Every input element is read exactly once (v[t+1] is the carried vnext, never a second load) and every thread reads row t of its
 * columns before it writes row t, so two in-place forms are defined: d_return == d_value with d_advantage == d_reward, and
 * d_advantage == d_value with d_return == d_reward (or either half of one).  Either output may be NULL, not both.
 * steps == 0 or count == 0: a successful no-op.  GYMNET_ERR_INVALID_ARG (message: gymnet_last_error) for negative sizes,
 * stride < count, a NULL d_reward / d_done, both outputs NULL, gamma or lambda not finite or outside [0, 1], a float pointer that is not
 * 4-byte aligned, and any other aliasing equal pointers show: d_advantage == d_return, an output equal to d_done / d_boot / d_last_value.
 * Nothing is written by a refused call. */
int gymnet_gae_device(int device, void *stream, int64_t steps, int64_t count, int64_t stride,
                      const float *d_reward, const uint8_t *d_done, const float *d_value, const float *d_last_value,
                      const float *d_boot, float gamma, float lambda, float *d_advantage, float *d_return);

/* ---- the network inputs of a recorded rollout (what the actions were chosen from: the input of an on-policy update) ----------
 * For step t of a lane: the lane's last S = `history` observations before the step, oldest first, clamped to the episode's first
 * observation — what gymnet_vecenv_actor_act_device read when it chose the action of step t.  Rebuilt from the rows a fused rollout
 * recorded (d_rec_obs, d_rec_done) and the history the rollout started from (gymnet_vecenv_actor_history_device, taken before it).
 * Handle-less like gymnet_gae_device: on `stream` of `device`, stream-ordered, non-blocking, capturable (no allocation, copy or
 * synchronise).  An added export: the ABI version stays 6.  Pure data movement, specified bit for bit.
 *     d_rec_obs  [steps][obs_dim][stride] float32, or float64 where obs_f64 != 0 (each value is then rounded to float32, to nearest even);
 *     d_rec_done [steps][stride] uint8;  stride >= count, lane i is column i;
 *     d_history0 [history][obs_dim][history0_stride] float32, oldest first: the input of step 0;
 *     d_x        output rows of history * obs_dim float32, x_row_stride floats apart (>= history * obs_dim; the floats between rows are
 *                not touched);  d_history_out (optional) [history][obs_dim][history_out_stride]: the history after the last step.
 * Per lane i: H_0 = column i of d_history0.  For t = 0 .. steps-1, with o = f32(d_rec_obs[t][:, i]) and d = d_rec_done[t][i]:
 *     the input of step t:  x[t][i][s * obs_dim + k] = H_t[s][k]                       s < history, k < obs_dim
 *     d != 0 (either bit):  every row of H_{t+1} = o
 *     otherwise:            H_{t+1}[s] = H_t[s+1] for s < history-1,  H_{t+1}[history-1] = o
 * This is the rule of gymnet_vecenv_actor_push_device: on a GYMNET_FLAG_AUTORESET handle d_rec_obs[t] is the new episode's first
 * observation on a done row, on any other handle the terminal one.  d_history_out = H_steps, so a rollout cut into two calls chains
 * (the second call's d_history0 is the first's d_history_out and its arrays start at row steps_1).
 * Values are copied as bit patterns: NaN payloads, -0.0 and denormals pass unchanged (float64 observations: one conversion).
 * Dense form (d_rows NULL; num_rows is not read): steps * count rows, row t * count + i at d_x + (t * count + i) * x_row_stride.
 * Gathered form (d_rows int64 [num_rows] on the device, flat row indices t * count + i): row d_rows[j] at d_x + j * x_row_stride.
 *   Duplicates are allowed.  The host cannot see the indices: one outside [0, steps * count) writes a row of canonical NaNs (0x7FC00000),
 *   and nothing outside row j is touched.  d_history_out is written as in the dense form.  num_rows == 0 is a no-op.
 * Accepted: obs_dim >= 1, history >= 1, history * obs_dim <= 64 (exactly the inputs an actor can have).  steps == 0 or count == 0 writes
 * only d_history_out = H_0 (in either form).
 * GYMNET_ERR_INVALID_ARG (message "rollout_inputs: ...": gymnet_last_error), nothing written: a negative size or stride; obs_dim,
 * history or their product outside the range; stride, history0_stride or (with d_history_out) history_out_stride below count;
 * x_row_stride below history * obs_dim where rows are to be written; a NULL d_rec_obs, d_rec_done or d_history0 with steps > 0, a NULL
 * d_history0 with d_history_out; a NULL d_x where rows are to be written; a pointer that is not 4-byte aligned (d_rec_obs with obs_f64
 * and d_rows: 8-byte; d_rec_done: any); d_x or d_history_out equal to an input pointer or to each other; sizes whose product leaves an
 * int64. */
int gymnet_rollout_inputs_device(int device, void *stream, int64_t steps, int64_t count, int64_t stride,
                                 int32_t obs_dim, int32_t history, int32_t obs_f64,
                                 const void *d_rec_obs, const uint8_t *d_rec_done,
                                 const float *d_history0, int64_t history0_stride,
                                 const int64_t *d_rows, int64_t num_rows,
                                 float *d_x, int64_t x_row_stride,
                                 float *d_history_out, int64_t history_out_stride);

/* ---- multi-GPU group: ONE process (e.g. a C# host) driving G members, one per GPU ----------------------------
 * The reference has no multi-device code; what shards is the independence of VecEnvWrapper's map (VecEnvWrapper.cs:22-24).
 * Member m owns the contiguous global lanes [m*N/G, (m+1)*N/G) (reset draws keyed by GLOBAL lane id: results do not depend
 * on G).  Every member keeps a replica of the whole batch's observations on its own GPU, rank-major [G][obs_dim][N/G]; the
 * member's live observation arrays ARE slice [m] of its replica (zero-copy send side).  gymnet_group_allgather_obs completes
 * the replicas:
 *   DIRECT  hand-written full-mesh push: each member stores its slice into the G-1 peers' replicas through peer-mapped
 *           memory, one peer per xGMI link, all links concurrently (~110 us for 16 MiB at 8 GPUs vs ~770 us for a ring);
 *   RCCL    ncclAllGather (in place) on per-member communicators (ncclCommInitAll); needs G distinct devices.
 * With GYMNET_FLAG_DOUBLE_BUFFER the gather runs on per-member side streams and overlaps the next step.
 * All calls are stream-ordered and non-blocking unless they take host buffers. */
typedef struct gymnet_group gymnet_group;
typedef enum gymnet_gather_mode { GYMNET_GATHER_NONE = 0, GYMNET_GATHER_DIRECT = 1, GYMNET_GATHER_RCCL = 2 } gymnet_gather_mode;

typedef struct gymnet_group_config {
    uint32_t struct_size;       /* = sizeof(gymnet_group_config) */
    int32_t  env_id;
    int64_t  global_num_envs;   /* N: lanes of the whole batch; a multiple of num_members */
    int32_t  num_members;       /* G, 1..16 */
    uint32_t flags;             /* GYMNET_FLAG_* for every member */
    uint64_t seed;
    const int32_t *devices;     /* [G] HIP device ordinal per member; NULL = 0..G-1.  An ordinal may repeat (several logical
                                   members on one GPU — how a 1-GPU box tests the path); RCCL needs distinct ordinals */
    int32_t  gather;            /* gymnet_gather_mode */
    int32_t  max_episode_steps;
} gymnet_group_config;

int gymnet_group_create(const gymnet_group_config *cfg, gymnet_group **out);
int gymnet_group_destroy(gymnet_group *g);
int gymnet_group_size(gymnet_group *g, int32_t *num_members, int64_t *lanes_per_member);
/* The member's handle (borrowed: destroyed with the group).  Everything gymnet_vecenv_* offers works on it. */
int gymnet_group_member(gymnet_group *g, int32_t member, gymnet_vecenv **out);
int gymnet_group_seed(gymnet_group *g, uint64_t seed);                        /* VecEnv.Seed(int), VecEnv.cs:44-46 */
int gymnet_group_reset_device(gymnet_group *g);                               /* VecEnv.Reset() on every member */
/* One vector step of the whole batch = one kernel launch per member.  d_actions[m]: pointer ON member m's device to that
 * member's N/G actions. */
int gymnet_group_step_device(gymnet_group *g, const void *const *d_actions);
/* `steps` vector steps per member (gymnet_vecenv_rollout_device on each, launches interleaved across members). */
int gymnet_group_rollout_device(gymnet_group *g, const void *const *d_actions, int64_t steps, int64_t action_stride, int64_t ring);
/* Completes every member's replica with the observations of the most recent step / reset.  Work queued on a member's stream
 * after gymnet_group_wait_gather (or, without DOUBLE_BUFFER, after this call) sees all G slices. */
int gymnet_group_allgather_obs(gymnet_group *g);
int gymnet_group_wait_gather(gymnet_group *g);
/* Member m's replica that was gathered last: device [G][obs_dim][N/G] on m's GPU — float32, or float64 when the group was created
 * with GYMNET_FLAG_F64 (here and in the three calls below). */
int gymnet_group_global_obs(gymnet_group *g, int32_t member, void **d_obs_all);
/* The same replica copied to the host, [G][obs_dim][N/G]; waits for the last gather and blocks. */
int gymnet_group_read_replica(gymnet_group *g, int32_t member, void *replica_out);
int gymnet_group_sync(gymnet_group *g);
/* Host-boundary forms over the whole batch (NDArray-shaped: obs [N, obs_dim], reward [N], done [N]; any may be NULL). */
int gymnet_group_reset(gymnet_group *g, void *obs_out);
int gymnet_group_step(gymnet_group *g, const void *actions, void *obs_out, float *reward_out, uint8_t *done_out);

/* ---- peer buffers: the direct all-gather for ONE PROCESS PER GPU hosts ---------------------------------------------
 * gymnet_group_* needs all GPUs in one process.  A host that runs one process per GPU (torch.distributed, MPI, a .NET
 * launcher) gets the same hand-written push over xGMI with these four calls: every rank creates its replica buffer
 * [G][obs_dim][N/G] as a peer buffer, hands the 64-byte handle to the other ranks by whatever channel it has, opens theirs,
 * creates its handle with d_ext_obs = buffer + rank * obs_dim * (N/G), and after a step pushes its slice into every
 * peer's replica.  Cross-process ordering is the host's: synchronize the stream, then a node barrier, before anyone reads a
 * replica or pushes into it again.  Teardown in the same spirit: barrier, every rank closes what it opened, barrier,
 * then every rank destroys what it created (no exporter frees memory a peer still has mapped).
 * (HIP IPC; needs HSA_ENABLE_IPC_MODE_LEGACY=0 on this platform's driver.) */
typedef struct gymnet_ipc_handle { char bytes[64]; } gymnet_ipc_handle;
int gymnet_peer_buffer_create(int device, int64_t bytes, void **d_ptr, gymnet_ipc_handle *handle);   /* hipMalloc + zero + export */
int gymnet_peer_buffer_open(int device, const gymnet_ipc_handle *handle, void **d_ptr);              /* map a peer's buffer */
int gymnet_peer_buffer_close(int device, void *d_ptr);                                               /* unmap an opened buffer */
int gymnet_peer_buffer_destroy(int device, void *d_ptr);                                             /* free a created buffer */
/* Stores `count` 4-byte words (floats; a float64 slice counts two per element) from d_src into the same-shaped slice d_dst[p] of every peer (p < npeers <= 15), all peers
 * concurrently (one grid row per peer = one xGMI link each), on `stream` (a hipStream_t of `device`; NULL = default): stream-ordered,
 * non-blocking, capturable (no allocation, copy or synchronise) — d_dst is a HOST array, read before the call returns; the peers' addresses
 * are kernel arguments, frozen by a capture. */
int gymnet_push_obs_device(int device, void *stream, const float *d_src, float *const *d_dst, int32_t npeers, int64_t count);

#ifdef __cplusplus
}
#endif
#endif /* GYMNET_AMD_H */
