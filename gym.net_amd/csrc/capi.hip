// capi.hip — the C ABI (include/gymnet_amd.h) over the HIP kernels.  Host code only; compiled by hipcc.  The launch policy, the
// resident mailbox, the graph-replay rollout and the fused rollout have units of their own (launch_policy.hip, resident.hip,
// step_graph.hip, rollout_fused.hip; handle.hpp); frame skip's entry points are in action_repeat.hip.
//
// There is NO CPU fallback in this library: without a usable AMD GPU every compute entry point fails
// with GYMNET_ERR_NO_DEVICE / GYMNET_ERR_HIP.  The CPU restatement under oracle/ is test infrastructure
// and is never linked here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "handle.hpp"

using namespace gymnet;

namespace {
thread_local std::string g_last_error;
constexpr int64_t kSmallHostPath = 4096;
constexpr float FMAX = 3.4028234663852886e38f;
constexpr float PI_F = 3.14159265358979323846f;
}  // namespace

namespace gymnet {

// Observation bounds: CartPoleEnv.cs:46-48 (high = [x_thr*2, float.MaxValue, theta_thr*2, float.MaxValue]).
// Algorithmic bytes per env-step: SURVEY.md §8(a)/(d).
const EnvDesc kEnvs[kNumEnvs] = {
    {"CartPole-v1", 4, 4, true, false, true, 2, 0.f, 0.f,
     {-4.8000002f, -FMAX, -0.41887903f, -FMAX}, {4.8000002f, FMAX, 0.41887903f, FMAX}, 0.f, 1.f, 41, 41, {-1, -1, -1, -1}},
    {"Pendulum-v1", 2, 3, false, true, false, 0, -2.f, 2.f,
     {-1.f, -1.f, -8.f}, {1.f, 1.f, 8.f}, -16.2736044f, 0.f, 37, 33, {-1, 2, -1, -1}},
    {"MountainCar-v0", 2, 2, true, false, false, 3, 0.f, 0.f,
     {-1.2f, -0.07f}, {0.6f, 0.07f}, -1.f, -1.f, 25, 25, {-1, -1, -1, -1}},
    {"Acrobot-v1", 4, 6, false, false, false, 3, 0.f, 0.f,
     {-1.f, -1.f, -1.f, -1.f, -4.f * PI_F, -9.f * PI_F}, {1.f, 1.f, 1.f, 1.f, 4.f * PI_F, 9.f * PI_F}, -1.f, 0.f, 65, 57, {-1, -1, 4, 5}},
    // reward (done ? 100 : 0) - 0.1 a^2 of the RAW action: unbounded below.  25 B per env-step like MountainCar: 8 state read, 4 action
    // read, 8 state written, 4 reward, 1 done
    {"MountainCarContinuous-v0", 2, 2, true, true, false, 0, -1.f, 1.f,
     {-1.2f, -0.07f}, {0.6f, 0.07f}, -INFINITY, 100.f, 25, 25, {-1, -1, -1, -1}},
};

void set_last_error(const char *msg) { g_last_error = msg ? msg : ""; }

int fail(gymnet_vecenv *h, int status, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    if (h) h->err = buf;
    // HIP keeps the last error of the calling thread until somebody reads it, and the launchers end with `return
    // hipGetLastError()`: a HIP failure reported here must not make the NEXT (valid) launch on this thread fail too.
    // A pure argument-validation failure made no HIP call and does not touch the runtime.
    if (status == GYMNET_ERR_HIP || status == GYMNET_ERR_OOM || status == GYMNET_ERR_RCCL) (void)hipGetLastError();
    return status;
}

}  // namespace gymnet

namespace {

template <class T>
int dalloc(gymnet_vecenv *h, T **p, size_t count) {
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, count * sizeof(T) + 16);
    if (e != hipSuccess) return fail(h, GYMNET_ERR_OOM, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
    h->owned.push_back(q);
    *p = static_cast<T *>(q);
    return GYMNET_OK;
}

// Host-boundary staging (actions in, row-major observations out, reset mask) is allocated on first use: a
// device-resident consumer (bench.py, a GPU policy) never pays for it — at 2^27 CartPole lanes it is 2.6 GiB.
int ensure_staging(gymnet_vecenv *h, bool actions, bool pack, bool mask) {
    if (actions && !h->d_actions) ST_TRY(dalloc(h, (int32_t **)&h->d_actions, (size_t)h->padded));
    if (pack && !h->d_pack) ST_TRY(dalloc(h, (char **)&h->d_pack, (size_t)h->padded * h->desc->obs_dim * h->esz));
    if (mask && !h->d_mask) ST_TRY(dalloc(h, &h->d_mask, (size_t)h->padded));
    return GYMNET_OK;
}

// Gathers the sharded done list of the most recent step — and the records written beside it — into compact arrays
// (stream-ordered, non-blocking); with `dense`, also applies the records to the dense per-lane arrays.  NULL outputs are skipped.
template <class R>
int compact_done_typed(gymnet_vecenv *h, int32_t *d_list, float *d_ret, int32_t *d_len, void *d_obs, int64_t capacity, uint32_t *d_count, bool dense) {
    CompactArgsT<R> c{};
    c.counts = h->d_done_count2 + (size_t)h->last_cparity * kShards * kCountStride;
    c.list = h->d_done_list; c.cap = h->done_cap;
    c.rec_ret = h->d_rec_ret; c.rec_len = h->d_rec_len; c.rec_obs = static_cast<const R *>(h->d_rec_obs); c.obs_dim = h->desc->obs_dim;
    c.out_list = d_list; c.out_ret = d_ret; c.out_len = d_len; c.out_obs = static_cast<R *>(d_obs); c.out_capacity = capacity; c.out_count = d_count;
    if (dense) { c.dense_ret = h->d_rec_ret ? h->d_fin_ret : nullptr; c.dense_len = h->d_fin_len; c.dense_obs = h->d_rec_obs ? static_cast<R *>(h->d_final_obs) : nullptr; }
    c.n = h->n;
    HIP_TRY(h, launch_compact_done(c, h->stream));
    return GYMNET_OK;
}
// d_obs: terminal observations of the handle's state scalar (float, or double for a GYMNET_FLAG_F64 handle)
int compact_done(gymnet_vecenv *h, int32_t *d_list, float *d_ret, int32_t *d_len, void *d_obs, int64_t capacity, uint32_t *d_count,
                 bool dense = false) {
    return h->f64 ? compact_done_typed<double>(h, d_list, d_ret, d_len, d_obs, capacity, d_count, dense)
                  : compact_done_typed<float>(h, d_list, d_ret, d_len, d_obs, capacity, d_count, dense);
}

// device address of state row k of the CURRENT state (its own row of d_state, or the observation row that holds it)
void *state_row(gymnet_vecenv *h, int k) {
    const int m = h->desc->alias ? -1 : h->desc->state_row_in_obs[k];
    return m < 0 ? row_at(h->d_state, k, h->sstride, h->esz) : row_at(h->d_obs, m, h->ostride, h->esz);
}

void recompute_extras(gymnet_vecenv *h) {
    h->extras = (h->cfg.flags & (GYMNET_FLAG_DONE_LIST | GYMNET_FLAG_EPISODE_STATS | GYMNET_FLAG_FINAL_OBS)) != 0 ||
                h->d_lane_seed != nullptr;
}

}  // namespace

namespace gymnet {

// Env.Seed(int) on a handle the caller has ENTERed
int seed_handle(gymnet_vecenv *h, uint64_t seed) {
    h->seed = seed;
    h->tick = 0;
    touch_epoch(h);
    drop_graphs(h);   // the seed is a (frozen) kernel argument of captured launches
    h->d_lane_seed = nullptr;   // back to one key for all lanes (d_lane_seed_buf is kept for the next Seed(int[]))
    recompute_extras(h);
    return write_tick(h);
}

// after a step launch with GYMNET_FLAG_DOUBLE_BUFFER: what was written becomes current
void swap_buffers(gymnet_vecenv *h) {
    if (!h->double_buffer) return;
    if (h->desc->alias) { std::swap(h->d_state, h->d_state_alt); h->d_obs = h->d_state; h->d_obs_alt = h->d_state_alt; }
    else std::swap(h->d_obs, h->d_obs_alt);
    h->cur ^= 1;
}

// one vector step = one kernel launch; bumps the host mirrors of the device-side counters
int launch_one_step(gymnet_vecenv *h, const void *d_actions) {
    int cparity;
    if (h->f64) {
        const StepArgsT<double> a = make_step_args<double>(h, d_actions);
        cparity = a.cparity;
        HIP_TRY(h, h->launch_f64->step(h->autoreset, h->extras, a, h->lcfg, h->stream));
    } else {
        const StepArgsT<float> a = make_step_args<float>(h, d_actions);
        cparity = a.cparity;
        HIP_TRY(h, h->launch_f32->step(h->autoreset, h->extras, a, h->lcfg, h->stream));
    }
    swap_buffers(h);
    h->last_cparity = cparity;
    h->tick += 1;
    h->tslot ^= 1;
    h->step_launches += 1;
    h->lane_steps += (uint64_t)h->n;
    return GYMNET_OK;
}

template <class R>
static int reset_lanes_typed(gymnet_vecenv *h, const uint8_t *d_mask) {
    HIP_TRY(h, launchers<R>(h).reset(make_reset_args<R>(h, d_mask), h->stream));
    h->tick += 1;
    touch_epoch(h);
    h->tslot ^= 1;
    return GYMNET_OK;
}

int launch_reset_lanes(gymnet_vecenv *h, const uint8_t *d_mask) {
    return h->f64 ? reset_lanes_typed<double>(h, d_mask) : reset_lanes_typed<float>(h, d_mask);
}

int write_tick(gymnet_vecenv *h) {
    uint64_t both[2] = {h->tick, h->tick};
    HIP_TRY(h, hipMemcpyAsync(h->d_tick2, both, sizeof both, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // `both` is a stack temporary
    return GYMNET_OK;
}

// row-major packing / host export of the CURRENT observations, typed by the handle's state scalar
static hipError_t pack_current_obs(gymnet_vecenv *h, const void *src_obs, int64_t stride, void *dst) {
    return h->f64 ? launch_pack_obs(h->desc->obs_dim, static_cast<const double *>(src_obs), stride, static_cast<double *>(dst), h->n, h->stream)
                  : launch_pack_obs(h->desc->obs_dim, static_cast<const float *>(src_obs), stride, static_cast<float *>(dst), h->n, h->stream);
}
static hipError_t export_current(gymnet_vecenv *h, bool host_form, void *obs_out, float *reward_out, uint8_t *done_out) {
    const int O = h->desc->obs_dim;
    if (h->f64) {
        const double *o = static_cast<const double *>(h->d_obs);
        return host_form ? launch_export_host(O, o, h->ostride, h->d_reward, h->d_done, static_cast<double *>(obs_out), reward_out, done_out, h->n, h->stream)
                         : launch_export_small(O, o, h->ostride, h->d_reward, h->d_done, static_cast<double *>(obs_out), reward_out, done_out, h->n, h->stream);
    }
    const float *o = static_cast<const float *>(h->d_obs);
    return host_form ? launch_export_host(O, o, h->ostride, h->d_reward, h->d_done, static_cast<float *>(obs_out), reward_out, done_out, h->n, h->stream)
                     : launch_export_small(O, o, h->ostride, h->d_reward, h->d_done, static_cast<float *>(obs_out), reward_out, done_out, h->n, h->stream);
}

// queues the copies of the current results to host buffers (any may be NULL) without the closing synchronize;
// only for handles without the host-mapped small-batch path
int queue_copy_out(gymnet_vecenv *h, void *obs_out, float *reward_out, uint8_t *done_out) {
    const EnvDesc &d = *h->desc;
    if (obs_out) {
        ST_TRY(ensure_staging(h, false, true, false));
        HIP_TRY(h, pack_current_obs(h, h->d_obs, h->ostride, h->d_pack));
        HIP_TRY(h, hipMemcpyAsync(obs_out, h->d_pack, (size_t)h->n * d.obs_dim * h->esz, hipMemcpyDeviceToHost, h->stream));
    }
    if (reward_out) HIP_TRY(h, hipMemcpyAsync(reward_out, h->d_reward, (size_t)h->n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (done_out) HIP_TRY(h, hipMemcpyAsync(done_out, h->d_done, (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
    return GYMNET_OK;
}

// copy the current results to host buffers (any may be NULL); blocks
int copy_out(gymnet_vecenv *h, void *obs_out, float *reward_out, uint8_t *done_out) {
    const EnvDesc &d = *h->desc;
    const size_t esz = h->esz;      // element size of an observation at the boundary
    if (h->pin_block && (obs_out || reward_out || done_out) && (!obs_out || obs_out == h->pin_obs) &&
        (!reward_out || reward_out == h->pin_reward) && (!done_out || done_out == h->pin_done)) {
        // the caller reads the library's pinned buffers: ONE kernel writes the results across PCIe, no staging, no memcpy calls
        HIP_TRY(h, export_current(h, /*host_form=*/true, obs_out, reward_out, done_out));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return GYMNET_OK;
    }
    if (h->hm_block) {   // latency path for small batches: one export kernel into host-mapped memory, one sync, host memcpy
        if (obs_out || reward_out || done_out)
            HIP_TRY(h, export_current(h, /*host_form=*/false, h->hm_obs, reward_out ? h->hm_reward : nullptr, done_out ? h->hm_done : nullptr));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (obs_out) std::memcpy(obs_out, h->hm_obs, (size_t)h->n * d.obs_dim * esz);
        if (reward_out) std::memcpy(reward_out, h->hm_reward, (size_t)h->n * sizeof(float));
        if (done_out) std::memcpy(done_out, h->hm_done, (size_t)h->n);
        return GYMNET_OK;
    }
    ST_TRY(queue_copy_out(h, obs_out, reward_out, done_out));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GYMNET_OK;
}

// Discrete.Contains over the staged batch (only with GYMNET_FLAG_VALIDATE_ACTIONS); blocks
int validate_staged_actions(gymnet_vecenv *h, const void *d_actions) {
    const EnvDesc &d = *h->desc;
    if (!(h->cfg.flags & GYMNET_FLAG_VALIDATE_ACTIONS) || d.box_action) return GYMNET_OK;
    uint32_t bad = 0;
    ST_TRY(count_bad_actions(h, 1, [&](int64_t) { return d_actions; }, &bad));
    if (bad)
        return fail(h, GYMNET_ERR_INVALID_ACTION, "Action is outside of the configured action space. (%u of %lld lanes, Discrete(%d))",
                    bad, (long long)h->n, d.action_n);
    return GYMNET_OK;
}

// stages host actions; *d_use receives the device-visible pointer the step kernel should read
int stage_host_actions(gymnet_vecenv *h, const void *actions, const void **d_use, bool validate_now) {
    if (!actions) return fail(h, GYMNET_ERR_INVALID_ARG, "actions is null");
    if (h->hm_block) {   // the previous step's kernel has completed (every host-boundary call ends with a sync)
        std::memcpy(h->hm_actions, actions, (size_t)h->n * 4);
        *d_use = h->hm_actions;
    } else {
        ST_TRY(ensure_staging(h, true, false, false));
        HIP_TRY(h, hipMemcpyAsync(h->d_actions, actions, (size_t)h->n * 4, hipMemcpyHostToDevice, h->stream));
        *d_use = h->d_actions;
    }
    return validate_now ? validate_staged_actions(h, *d_use) : GYMNET_OK;
}

}  // namespace gymnet

extern "C" {

int gymnet_abi_version(void) { return GYMNET_ABI_VERSION; }

const char *gymnet_status_string(int status) {
    switch (status) {
        case GYMNET_OK: return "ok";
        case GYMNET_ERR_INVALID_ARG: return "invalid argument";
        case GYMNET_ERR_INVALID_ACTION: return "Action is outside of the configured action space.";
        case GYMNET_ERR_HIP: return "HIP runtime error";
        case GYMNET_ERR_OOM: return "out of memory";
        case GYMNET_ERR_NO_DEVICE: return "no AMD GPU available (this engine has no CPU fallback)";
        case GYMNET_ERR_ALREADY_STEPPING: return "already running an async step";
        case GYMNET_ERR_NOT_STEPPING: return "not running an async step";
        case GYMNET_ERR_UNSUPPORTED: return "unsupported for this environment / configuration";
        case GYMNET_ERR_RCCL: return "RCCL error";
        default: return "unknown status";
    }
}

const char *gymnet_last_error(void) { return g_last_error.c_str(); }

int gymnet_device_count(int *count) {
    return guarded([&]() -> int {
    if (!count) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "count is null");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess || c <= 0) {
        *count = 0;
        (void)hipGetLastError();
        return fail(nullptr, GYMNET_ERR_NO_DEVICE, "hipGetDeviceCount: %s", e == hipSuccess ? "0 devices" : hipGetErrorString(e));
    }
    *count = c;
    return GYMNET_OK;
    });
}

int gymnet_env_describe(int env_id, gymnet_env_info *out) {
    return guarded([&]() -> int {
    if (!out) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "out is null");
    if (env_id < 0 || env_id >= kNumEnvs) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "unknown env_id %d", env_id);
    const EnvDesc &d = kEnvs[env_id];
    std::memset(out, 0, sizeof *out);
    out->struct_size = sizeof *out;
    out->env_id = env_id;
    std::snprintf(out->name, sizeof out->name, "%s", d.name);
    out->state_dim = d.state_dim; out->obs_dim = d.obs_dim; out->obs_aliases_state = d.alias;
    out->action_is_box = d.box_action; out->action_n = d.action_n;
    out->action_low = d.action_low; out->action_high = d.action_high;
    for (int k = 0; k < 8; ++k) { out->obs_low[k] = d.obs_low[k]; out->obs_high[k] = d.obs_high[k]; }
    out->reward_low = d.reward_low; out->reward_high = d.reward_high;
    out->algorithmic_bytes_per_step = d.algorithmic_bytes;
    out->traffic_bytes_per_step = d.traffic_bytes;
    for (int k = 0; k < 8; ++k) out->state_row_in_obs[k] = (k < d.state_dim && !d.alias) ? d.state_row_in_obs[k] : -1;
    return GYMNET_OK;
    });
}

int gymnet_vecenv_destroy(gymnet_vecenv *h) {
    return guarded([&]() -> int {
    if (!h) return GYMNET_OK;
    DeviceScope dev_scope;
    (void)hipSetDevice(h->device);
    resident_release(h);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    drop_graphs(h);
    for (void *p : h->owned) (void)hipFree(p);
    if (h->ep.d) (void)hipFree(h->ep.d);
    (void)release_render(h); (void)release_stack(h); (void)release_memory(h); (void)release_actor(h);
    if (h->hm_block) (void)hipHostFree(h->hm_block);
    if (h->pin_block) (void)hipHostFree(h->pin_block);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return GYMNET_OK;
    });
}

int gymnet_vecenv_create(const gymnet_config *cfg, gymnet_vecenv **out) {
    return guarded([&]() -> int {
    if (!out) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    if (!cfg) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "cfg is null");
    if (cfg->struct_size != sizeof(gymnet_config))
        return fail(nullptr, GYMNET_ERR_INVALID_ARG, "cfg.struct_size %u != %zu (ABI mismatch)", cfg->struct_size, sizeof(gymnet_config));
    if (cfg->env_id < 0 || cfg->env_id >= kNumEnvs) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "unknown env_id %d", cfg->env_id);
    if (cfg->num_envs <= 0 || cfg->num_envs > (int64_t)1 << 31)
        return fail(nullptr, GYMNET_ERR_INVALID_ARG, "num_envs %lld out of range [1, 2^31]", (long long)cfg->num_envs);
    if (cfg->lane_offset < 0) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "lane_offset < 0");
    constexpr uint32_t kKnownFlags = GYMNET_FLAG_AUTORESET | GYMNET_FLAG_VALIDATE_ACTIONS | GYMNET_FLAG_DONE_LIST | GYMNET_FLAG_EPISODE_STATS |
                                     GYMNET_FLAG_FINAL_OBS | GYMNET_FLAG_DOUBLE_BUFFER | GYMNET_FLAG_F64 | GYMNET_FLAG_COMPACT_RECORDS_ONLY |
                                     GYMNET_FLAG_RESIDENT;
    if (cfg->flags & ~kKnownFlags)      // a flag from a newer header must not be silently ignored by an older library
        return fail(nullptr, GYMNET_ERR_INVALID_ARG, "unknown flag bits 0x%x (this library is ABI %d)", cfg->flags & ~kKnownFlags, GYMNET_ABI_VERSION);
    if (cfg->max_episode_steps < 0 || (cfg->max_episode_steps > 0 && !(cfg->flags & GYMNET_FLAG_EPISODE_STATS)))
        return fail(nullptr, GYMNET_ERR_INVALID_ARG, "max_episode_steps needs GYMNET_FLAG_EPISODE_STATS");
    if ((cfg->flags & GYMNET_FLAG_FINAL_OBS) && !(cfg->flags & GYMNET_FLAG_AUTORESET))
        return fail(nullptr, GYMNET_ERR_INVALID_ARG, "GYMNET_FLAG_FINAL_OBS needs GYMNET_FLAG_AUTORESET");
    if (cfg->d_ext_obs && cfg->ext_obs_stride < cfg->num_envs)
        return fail(nullptr, GYMNET_ERR_INVALID_ARG, "ext_obs_stride %lld < num_envs", (long long)cfg->ext_obs_stride);
    if (cfg->d_ext_obs_alt && (!cfg->d_ext_obs || !(cfg->flags & GYMNET_FLAG_DOUBLE_BUFFER)))
        return fail(nullptr, GYMNET_ERR_INVALID_ARG, "d_ext_obs_alt needs d_ext_obs and GYMNET_FLAG_DOUBLE_BUFFER");
    if (cfg->d_ext_obs_alt && cfg->d_ext_obs_alt == cfg->d_ext_obs)
        return fail(nullptr, GYMNET_ERR_INVALID_ARG, "d_ext_obs_alt must be a different buffer than d_ext_obs");
    if ((cfg->flags & GYMNET_FLAG_F64) && cfg->env_id != GYMNET_ENV_CARTPOLE)
        return fail(nullptr, GYMNET_ERR_UNSUPPORTED, "GYMNET_FLAG_F64 exists for CartPole only (the one env whose float64 arithmetic the reference defines)");
    const size_t esz_cfg = (cfg->flags & GYMNET_FLAG_F64) ? 8 : 4;
    if ((cfg->d_ext_obs && !aligned_to(cfg->d_ext_obs, (int)esz_cfg)) || (cfg->d_ext_obs_alt && !aligned_to(cfg->d_ext_obs_alt, (int)esz_cfg)))
        return fail(nullptr, GYMNET_ERR_INVALID_ARG, "d_ext_obs / d_ext_obs_alt must be aligned to the observation element (%zu bytes)", esz_cfg);
    if (cfg->flags & GYMNET_FLAG_RESIDENT) {
        if (cfg->num_envs > kMailboxLanes) return fail(nullptr, GYMNET_ERR_UNSUPPORTED, "GYMNET_FLAG_RESIDENT serves up to %d lanes (one wave)", kMailboxLanes);
        if ((cfg->flags & (GYMNET_FLAG_DONE_LIST | GYMNET_FLAG_FINAL_OBS | GYMNET_FLAG_DOUBLE_BUFFER)) || cfg->d_ext_obs || cfg->stream)
            return fail(nullptr, GYMNET_ERR_UNSUPPORTED, "GYMNET_FLAG_RESIDENT cannot be combined with DONE_LIST / FINAL_OBS / DOUBLE_BUFFER / d_ext_obs / a caller's stream");
    }
    if ((cfg->flags & GYMNET_FLAG_COMPACT_RECORDS_ONLY) && !(cfg->flags & GYMNET_FLAG_DONE_LIST))
        return fail(nullptr, GYMNET_ERR_INVALID_ARG, "GYMNET_FLAG_COMPACT_RECORDS_ONLY needs GYMNET_FLAG_DONE_LIST");

    int ndev = 0;
    int s = gymnet_device_count(&ndev);
    if (s != GYMNET_OK) return s;
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "device %d not in [0, %d)", cfg->device, ndev);

    gymnet_vecenv *h = new (std::nothrow) gymnet_vecenv();
    if (!h) return fail(nullptr, GYMNET_ERR_OOM, "host allocation failed");
    h->cfg = *cfg;
    h->desc = &kEnvs[cfg->env_id];
    h->device = cfg->device;
    h->n = cfg->num_envs;
    h->seed = cfg->seed;
    h->autoreset = (cfg->flags & GYMNET_FLAG_AUTORESET) != 0;
    h->double_buffer = (cfg->flags & GYMNET_FLAG_DOUBLE_BUFFER) != 0;
    h->f64 = (cfg->flags & GYMNET_FLAG_F64) != 0;
    h->esz = h->f64 ? 8 : 4;
    // (cfg.env_id and GYMNET_FLAG_F64 were checked above: the table exists)
    if (h->f64) h->launch_f64 = env_launchers<double>(cfg->env_id); else h->launch_f32 = env_launchers<float>(cfg->env_id);
    h->compact_only = (cfg->flags & GYMNET_FLAG_COMPACT_RECORDS_ONLY) != 0;
    const EnvDesc &d = *h->desc;
    DeviceScope dev_scope;

#define CREATE_TRY(expr)                      \
    do {                                      \
        int s_ = (expr);                      \
        if (s_ != GYMNET_OK) { gymnet_vecenv_destroy(h); return s_; } \
    } while (0)
#define CREATE_HIP(expr)                                                                    \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            int s_ = fail(nullptr, GYMNET_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
            gymnet_vecenv_destroy(h);                                                       \
            return s_;                                                                      \
        }                                                                                   \
    } while (0)

    CREATE_HIP(hipSetDevice(h->device));
    {   // SIMD units of this device: the launch policy's waves-per-SIMD arithmetic (default_policy) and the looped multi-pair kernel's
        // resident generation (pipe2_shape) are sized from the device the handle lives on, not from an MI355X literal
        int cus = 0;
        CREATE_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
        h->simds = cus > 0 ? cus * 4 : 1024;
    }
    if (cfg->stream) { h->stream = static_cast<hipStream_t>(cfg->stream); }
    else { CREATE_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)); h->own_stream = true; }

    const int64_t padded = (h->n + 63) / 64 * 64;   // every component array starts 256-byte aligned
    h->padded = padded;
    const size_t esz = h->esz;      // bytes per state / observation element: 4, or 8 for a GYMNET_FLAG_F64 handle
    if (cfg->d_ext_obs) {
        if (d.alias) { h->d_state = cfg->d_ext_obs; h->sstride = cfg->ext_obs_stride; h->d_obs = h->d_state; h->ostride = h->sstride; }
        else {
            h->d_obs = cfg->d_ext_obs; h->ostride = cfg->ext_obs_stride;
            CREATE_TRY(dalloc(h, (char **)&h->d_state, (size_t)padded * d.state_dim * esz)); h->sstride = padded;
        }
    } else {
        CREATE_TRY(dalloc(h, (char **)&h->d_state, (size_t)padded * d.state_dim * esz)); h->sstride = padded;
        if (d.alias) { h->d_obs = h->d_state; h->ostride = h->sstride; }
        else { CREATE_TRY(dalloc(h, (char **)&h->d_obs, (size_t)padded * d.obs_dim * esz)); h->ostride = padded; }
    }
    if (h->double_buffer) {   // the second observation buffer (for aliasing envs: the second STATE buffer), same stride
        void *alt = cfg->d_ext_obs_alt;
        if (!alt) CREATE_TRY(dalloc(h, (char **)&alt, (size_t)h->ostride * d.obs_dim * esz));
        if (d.alias) { h->d_state_alt = alt; h->d_obs_alt = alt; } else { h->d_obs_alt = alt; }
    }
    CREATE_TRY(dalloc(h, &h->d_reward, (size_t)padded));
    CREATE_TRY(dalloc(h, &h->d_done, (size_t)padded));
    CREATE_TRY(dalloc(h, &h->d_tick2, 2));
    // d_actions / d_pack / d_mask (host-boundary staging) are allocated on first use: ensure_staging()
    CREATE_TRY(dalloc(h, &h->d_after_done, (size_t)kShards * kAfterStride));
    CREATE_TRY(dalloc(h, &h->d_bad, 1));
    if (h->n <= kSmallHostPath) {
        const size_t a_bytes = (size_t)padded * 4, o_bytes = (size_t)padded * d.obs_dim * esz, r_bytes = (size_t)padded * 4, d_bytes = (size_t)padded;
        if (hipHostMalloc(&h->hm_block, a_bytes + o_bytes + r_bytes + d_bytes, hipHostMallocMapped) == hipSuccess) {
            char *b = static_cast<char *>(h->hm_block);
            h->hm_actions = b; h->hm_obs = b + a_bytes;
            h->hm_reward = reinterpret_cast<float *>(b + a_bytes + o_bytes); h->hm_done = reinterpret_cast<uint8_t *>(b + a_bytes + o_bytes + r_bytes);
        } else {
            (void)hipGetLastError();
            h->hm_block = nullptr;             // fall back to the memcpy path
        }
    }
    if (cfg->flags & GYMNET_FLAG_RESIDENT) CREATE_TRY(resident_create(h));
    if (d.has_sbd && !h->autoreset) CREATE_TRY(dalloc(h, &h->d_sbd, (size_t)padded));
    if (cfg->flags & GYMNET_FLAG_FINAL_OBS) CREATE_TRY(dalloc(h, (char **)&h->d_final_obs, (size_t)h->n * d.obs_dim * esz));
    if (cfg->flags & GYMNET_FLAG_DONE_LIST) {
        // segment capacity: the most lanes the waves of one shard can own, for any lane width (4 / 2 / 1 lanes per thread)
        const int64_t w4 = (h->n + 255) / 256, w2 = (h->n + 127) / 128, w1 = (h->n + 63) / 64;
        const int64_t cap4 = (w4 + kShards - 1) / kShards * 256, cap2 = (w2 + kShards - 1) / kShards * 128, cap1 = (w1 + kShards - 1) / kShards * 64;
        h->done_cap = cap4 > cap1 ? cap4 : cap1;
        if (cap2 > h->done_cap) h->done_cap = cap2;
        CREATE_TRY(dalloc(h, &h->d_done_list, (size_t)kShards * (size_t)h->done_cap));
        CREATE_TRY(dalloc(h, &h->d_done_compact, (size_t)padded));
        CREATE_TRY(dalloc(h, &h->d_done_count2, (size_t)2 * kShards * kCountStride));
        CREATE_TRY(dalloc(h, &h->d_done_total, 1));
        CREATE_HIP(hipMemsetAsync(h->d_done_count2, 0, (size_t)2 * kShards * kCountStride * sizeof(uint32_t), h->stream));
        CREATE_HIP(hipMemsetAsync(h->d_done_total, 0, sizeof(uint32_t), h->stream));
    }
    if ((cfg->flags & GYMNET_FLAG_DONE_LIST) && (cfg->flags & GYMNET_FLAG_EPISODE_STATS)) {
        CREATE_TRY(dalloc(h, &h->d_rec_ret, (size_t)kShards * (size_t)h->done_cap));
        CREATE_TRY(dalloc(h, &h->d_rec_len, (size_t)kShards * (size_t)h->done_cap));
    }
    if ((cfg->flags & GYMNET_FLAG_DONE_LIST) && (cfg->flags & GYMNET_FLAG_FINAL_OBS))
        CREATE_TRY(dalloc(h, (char **)&h->d_rec_obs, (size_t)kShards * (size_t)h->done_cap * d.obs_dim * esz));
    if (cfg->flags & GYMNET_FLAG_EPISODE_STATS) {
        CREATE_TRY(dalloc(h, &h->d_ep_ret, (size_t)padded)); CREATE_TRY(dalloc(h, &h->d_ep_len, (size_t)padded));
        CREATE_TRY(dalloc(h, &h->d_fin_ret, (size_t)padded)); CREATE_TRY(dalloc(h, &h->d_fin_len, (size_t)padded));
        CREATE_HIP(hipMemsetAsync(h->d_ep_ret, 0, (size_t)padded * 4, h->stream));
        CREATE_HIP(hipMemsetAsync(h->d_ep_len, 0, (size_t)padded * 4, h->stream));
        CREATE_HIP(hipMemsetAsync(h->d_fin_ret, 0, (size_t)padded * 4, h->stream));
        CREATE_HIP(hipMemsetAsync(h->d_fin_len, 0, (size_t)padded * 4, h->stream));
    }
    recompute_extras(h);
    // defined start: zero state, reward, done; sbd = -1
    CREATE_HIP(hipMemsetAsync(h->d_state, 0, ((size_t)h->sstride * (d.state_dim - 1) + (size_t)h->n) * esz, h->stream));
    if (!d.alias) CREATE_HIP(hipMemsetAsync(h->d_obs, 0, ((size_t)h->ostride * (d.obs_dim - 1) + (size_t)h->n) * esz, h->stream));
    if (h->d_obs_alt) CREATE_HIP(hipMemsetAsync(h->d_obs_alt, 0, ((size_t)h->ostride * (d.obs_dim - 1) + (size_t)h->n) * esz, h->stream));
    CREATE_HIP(hipMemsetAsync(h->d_reward, 0, (size_t)padded * 4, h->stream));
    CREATE_HIP(hipMemsetAsync(h->d_done, 0, (size_t)padded, h->stream));
    CREATE_HIP(hipMemsetAsync(h->d_after_done, 0, (size_t)kShards * kAfterStride * sizeof(unsigned long long), h->stream));
    if (h->d_final_obs) CREATE_HIP(hipMemsetAsync(h->d_final_obs, 0, (size_t)h->n * d.obs_dim * esz, h->stream));
    if (h->d_sbd) CREATE_HIP(launch_fill_i32(h->d_sbd, -1, h->n, h->stream));
    CREATE_TRY(write_tick(h));

    default_policy(h);
#undef CREATE_TRY
#undef CREATE_HIP
    *out = h;
    return GYMNET_OK;
    });
}

int gymnet_vecenv_seed(gymnet_vecenv *h, uint64_t seed) {
    return guarded([&]() -> int {
    ENTER(h);
    return seed_handle(h, seed);
    });
}

int gymnet_vecenv_seed_lanes(gymnet_vecenv *h, const uint64_t *seeds, int64_t count) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!seeds) return fail(h, GYMNET_ERR_INVALID_ARG, "seeds is null");
    if (count != h->n)   // VecEnv.cs:49
        return fail(h, GYMNET_ERR_INVALID_ARG, "Number of seeds passed should be equals to number of environments (%lld != %lld)",
                    (long long)count, (long long)h->n);
    // VecEnv.Seed(int) reaches a VecEnv-typed caller's lanes as N EQUAL seeds (VecEnv.cs:44-46 -> Environments[i].Seed(seed)).
    // With one key for every lane the per-lane-key kernel variant would compute exactly what the lean one does (the Philox
    // counter carries the lane id either way) — only slower, and without the fused rollout.  So an all-equal vector IS Seed(int).
    bool all_equal = true;
    for (int64_t i = 1; i < count && all_equal; ++i) all_equal = seeds[i] == seeds[0];
    if (all_equal) return seed_handle(h, seeds[0]);
    // one allocation, reused by every later Seed(int[]) (it used to grow by N*8 bytes per call); the stream is drained
    // first so no launch still in flight reads the keys being overwritten
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (!h->d_lane_seed_buf) ST_TRY(dalloc(h, &h->d_lane_seed_buf, (size_t)h->n));
    HIP_TRY(h, hipMemcpyAsync(h->d_lane_seed_buf, seeds, (size_t)h->n * 8, hipMemcpyHostToDevice, h->stream));
    h->d_lane_seed = h->d_lane_seed_buf;
    recompute_extras(h);
    h->tick = 0;
    touch_epoch(h);
    drop_graphs(h);
    return write_tick(h);   // synchronizes: `seeds` is the caller's again on return
    });
}

int gymnet_vecenv_reset_device(gymnet_vecenv *h) {
    return guarded([&]() -> int {
    ENTER(h);
    return launch_reset_lanes(h, nullptr);
    });
}

int gymnet_vecenv_reset_where_device(gymnet_vecenv *h, const uint8_t *d_mask) {
    return guarded([&]() -> int {
    ENTER(h);
    // with AUTORESET the step already re-drew every finished lane (its done flag stays set as the step's RESULT):
    // resetting "the lanes whose done flag is set" again would discard the observation the step returned
    if (!d_mask && h->autoreset) return GYMNET_OK;
    // own done flags: the reset kernel may read its mask from the very array it clears (each lane's flag is read
    // before the same thread clears it), so no snapshot copy is needed
    return launch_reset_lanes(h, d_mask ? d_mask : h->d_done);
    });
}

int gymnet_vecenv_reset(gymnet_vecenv *h, void *obs_out) {
    return guarded([&]() -> int {
    ENTER_KEEP_RESIDENT(h);
    if (resident_serves(h)) return resident_command(h, kMailboxResetAll, nullptr, obs_out, nullptr, nullptr);
    if (h->res.running) ST_TRY(resident_stop(h));
    ST_TRY(launch_reset_lanes(h, nullptr));
    return copy_out(h, obs_out, nullptr, nullptr);
    });
}

int gymnet_vecenv_reset_where(gymnet_vecenv *h, const uint8_t *mask, void *obs_out) {
    return guarded([&]() -> int {
    ENTER_KEEP_RESIDENT(h);
    if (!mask && !h->autoreset && resident_serves(h)) return resident_command(h, kMailboxResetDone, nullptr, obs_out, nullptr, nullptr);
    if (h->res.running) ST_TRY(resident_stop(h));
    if (!mask && h->autoreset) return copy_out(h, obs_out, nullptr, nullptr);   // no-op, see gymnet_vecenv_reset_where_device
    if (mask) {
        ST_TRY(ensure_staging(h, false, false, true));
        HIP_TRY(h, hipMemcpyAsync(h->d_mask, mask, (size_t)h->n, hipMemcpyHostToDevice, h->stream));
    }
    ST_TRY(launch_reset_lanes(h, mask ? h->d_mask : h->d_done));
    return copy_out(h, obs_out, nullptr, nullptr);
    });
}

int gymnet_vecenv_host_buffers(gymnet_vecenv *h, void **actions, void **obs, float **reward, uint8_t **done) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!h->pin_block) {
        const EnvDesc &d = *h->desc;
        auto up = [](size_t b) { return (b + 4095) & ~(size_t)4095; };          // every buffer on its own page
        const size_t a_b = up((size_t)h->n * 4), o_b = up((size_t)h->n * d.obs_dim * h->esz), r_b = up((size_t)h->n * 4), d_b = up((size_t)h->n);
        void *blk = nullptr;
        hipError_t e = hipHostMalloc(&blk, a_b + o_b + r_b + d_b, hipHostMallocMapped | hipHostMallocPortable);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, GYMNET_ERR_OOM, "hipHostMalloc(%zu bytes, mapped) failed: %s", a_b + o_b + r_b + d_b, hipGetErrorString(e)); }
        std::memset(blk, 0, a_b + o_b + r_b + d_b);
        char *b = static_cast<char *>(blk);
        h->pin_block = blk; h->pin_actions = b; h->pin_obs = b + a_b;
        h->pin_reward = reinterpret_cast<float *>(b + a_b + o_b); h->pin_done = reinterpret_cast<uint8_t *>(b + a_b + o_b + r_b);
    }
    if (actions) *actions = h->pin_actions;
    if (obs) *obs = h->pin_obs;
    if (reward) *reward = h->pin_reward;
    if (done) *done = h->pin_done;
    return GYMNET_OK;
    });
}

// Discrete.Contains over a HOST batch (the resident path validates before it posts: nothing has been staged on the device)
static int validate_host_actions(gymnet_vecenv *h, const void *actions) {
    const EnvDesc &d = *h->desc;
    if (!(h->cfg.flags & GYMNET_FLAG_VALIDATE_ACTIONS) || d.box_action) return GYMNET_OK;
    const int32_t *a = static_cast<const int32_t *>(actions);
    uint32_t bad = 0;
    for (int64_t i = 0; i < h->n; ++i) bad += (a[i] < 0 || a[i] >= d.action_n) ? 1u : 0u;
    if (bad) return fail(h, GYMNET_ERR_INVALID_ACTION, "Action is outside of the configured action space. (%u of %lld lanes, Discrete(%d))", bad, (long long)h->n, d.action_n);
    return GYMNET_OK;
}

int gymnet_vecenv_step(gymnet_vecenv *h, const void *actions, void *obs_out, float *reward_out, uint8_t *done_out) {
    return guarded([&]() -> int {
    ENTER_KEEP_RESIDENT(h);
    if (h->async_pending) return fail(h, GYMNET_ERR_ALREADY_STEPPING, "already running an async step");
    if (resident_serves(h)) {
        if (!actions) return fail(h, GYMNET_ERR_INVALID_ARG, "actions is null");
        ST_TRY(validate_host_actions(h, actions));
        return resident_command(h, kMailboxStep, actions, obs_out, reward_out, done_out);
    }
    const void *d_act = nullptr;
    ST_TRY(stage_host_actions(h, actions, &d_act, true));
    ST_TRY(launch_one_step(h, d_act));
    return copy_out(h, obs_out, reward_out, done_out);
    });
}

int gymnet_vecenv_step_broadcast(gymnet_vecenv *h, int32_t action, void *obs_out, float *reward_out, uint8_t *done_out) {
    return guarded([&]() -> int {
    ENTER_KEEP_RESIDENT(h);
    if (h->async_pending) return fail(h, GYMNET_ERR_ALREADY_STEPPING, "already running an async step");
    const EnvDesc &d = *h->desc;
    if (resident_serves(h)) {
        int32_t bits[kMailboxLanes];
        float f = (float)action;                         // IVecEnv.Step(int) on a Box space: the int is the (scalar) torque
        int32_t word = action;
        if (d.box_action) std::memcpy(&word, &f, 4);
        for (int64_t i = 0; i < h->n; ++i) bits[i] = word;
        ST_TRY(validate_host_actions(h, bits));
        return resident_command(h, kMailboxStep, bits, obs_out, reward_out, done_out);
    }
    ST_TRY(ensure_staging(h, true, false, false));
    if (d.box_action) {   // IVecEnv.Step(int) on a Box space: the int is the (scalar) torque
        float f = (float)action;
        int32_t bits;
        std::memcpy(&bits, &f, 4);
        HIP_TRY(h, launch_fill_i32(static_cast<int32_t *>(h->d_actions), bits, h->n, h->stream));
    } else {
        if ((h->cfg.flags & GYMNET_FLAG_VALIDATE_ACTIONS) && (action < 0 || action >= d.action_n))
            return fail(h, GYMNET_ERR_INVALID_ACTION, "Action is outside of the configured action space. (%d, Discrete(%d))", action, d.action_n);
        HIP_TRY(h, launch_fill_i32(static_cast<int32_t *>(h->d_actions), action, h->n, h->stream));
    }
    ST_TRY(launch_one_step(h, h->d_actions));
    return copy_out(h, obs_out, reward_out, done_out);
    });
}

int gymnet_vecenv_step_async(gymnet_vecenv *h, const void *actions) {
    return guarded([&]() -> int {
    ENTER(h);
    if (h->async_pending) return fail(h, GYMNET_ERR_ALREADY_STEPPING, "already running an async step");
    const void *d_act = nullptr;
    ST_TRY(stage_host_actions(h, actions, &d_act, true));
    ST_TRY(launch_one_step(h, d_act));
    h->async_pending = true;
    return GYMNET_OK;
    });
}

int gymnet_vecenv_step_wait(gymnet_vecenv *h, void *obs_out, float *reward_out, uint8_t *done_out) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!h->async_pending) return fail(h, GYMNET_ERR_NOT_STEPPING, "not running an async step");
    h->async_pending = false;
    return copy_out(h, obs_out, reward_out, done_out);
    });
}

int gymnet_vecenv_read(gymnet_vecenv *h, void *obs_out, float *reward_out, uint8_t *done_out) {
    return guarded([&]() -> int {
    ENTER(h);
    return copy_out(h, obs_out, reward_out, done_out);
    });
}

int gymnet_vecenv_step_device(gymnet_vecenv *h, const void *d_actions) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!d_actions) return fail(h, GYMNET_ERR_INVALID_ARG, "d_actions is null");
    if (h->lcfg.vec > 1 && !aligned_to(d_actions, 4 * h->lcfg.vec))
        return fail(h, GYMNET_ERR_INVALID_ARG, "d_actions must be %d-byte aligned", 4 * h->lcfg.vec);
    ST_TRY(validate_staged_actions(h, d_actions));
    return launch_one_step(h, d_actions);
    });
}

int gymnet_vecenv_rollout_device(gymnet_vecenv *h, const void *d_actions, int64_t steps, int64_t action_stride, int64_t ring) {
    return guarded([&]() -> int {
    ENTER(h);
    return rollout_steps(h, d_actions, steps, action_stride, ring);
    });
}

int gymnet_vecenv_pack_obs_device(gymnet_vecenv *h, void *d_obs_rowmajor) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!d_obs_rowmajor) return fail(h, GYMNET_ERR_INVALID_ARG, "d_obs_rowmajor is null");
    if (!aligned16(d_obs_rowmajor)) return fail(h, GYMNET_ERR_INVALID_ARG, "d_obs_rowmajor must be 16-byte aligned");
    HIP_TRY(h, pack_current_obs(h, h->d_obs, h->ostride, d_obs_rowmajor));
    return GYMNET_OK;
    });
}

int gymnet_vecenv_sync(gymnet_vecenv *h) {
    return guarded([&]() -> int {
    ENTER(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GYMNET_OK;
    });
}

int gymnet_vecenv_device_view(gymnet_vecenv *h, gymnet_device_view *out) {
    return guarded([&]() -> int {
    if (!h || !out) return fail(h, GYMNET_ERR_INVALID_ARG, "null argument");
    std::memset(out, 0, sizeof *out);
    out->struct_size = sizeof *out;
    out->state_dim = h->desc->state_dim; out->obs_dim = h->desc->obs_dim; out->obs_aliases_state = h->desc->alias;
    out->num_envs = h->n; out->state_stride = h->sstride; out->obs_stride = h->ostride;
    out->d_state = h->d_state; out->d_obs = h->d_obs;
    out->state_dtype = h->f64 ? GYMNET_DTYPE_F64 : GYMNET_DTYPE_F32;
    out->d_reward = h->d_reward; out->d_done = h->d_done;
    out->d_steps_beyond_done = h->d_sbd; out->d_final_obs = h->d_final_obs; out->d_done_list = h->d_done_compact;
    out->d_episode_return = h->d_ep_ret; out->d_episode_length = h->d_ep_len;
    out->d_finished_return = h->d_fin_ret; out->d_finished_length = h->d_fin_len;
    out->stream = h->stream;
    out->obs_buffer = h->cur;
    out->d_obs_alt = h->d_obs_alt;
    return GYMNET_OK;
    });
}

int gymnet_vecenv_get_state(gymnet_vecenv *h, void *state_soa_v) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!state_soa_v) return fail(h, GYMNET_ERR_INVALID_ARG, "state_soa is null");
    const size_t row = (size_t)h->n * h->esz;
    for (int k = 0; k < h->desc->state_dim; ++k)      // row by row: a row the observation repeats lives in the observation array
        HIP_TRY(h, hipMemcpyAsync(static_cast<char *>(state_soa_v) + (size_t)k * row, state_row(h, k), row, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GYMNET_OK;
    });
}

int gymnet_vecenv_set_state(gymnet_vecenv *h, const void *state_soa_v) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!state_soa_v) return fail(h, GYMNET_ERR_INVALID_ARG, "state_soa is null");
    const size_t row = (size_t)h->n * h->esz;
    touch_epoch(h);           // (before the first copy: a call that fails half way has changed observations too)
    for (int k = 0; k < h->desc->state_dim; ++k)
        HIP_TRY(h, hipMemcpyAsync(state_row(h, k), static_cast<const char *>(state_soa_v) + (size_t)k * row, row, hipMemcpyHostToDevice, h->stream));
    if (!h->desc->alias)      // (float32 envs only: the float64 handle's observation IS its state)
        HIP_TRY(h, h->launch_f32->observe(static_cast<const float *>(h->d_state), h->sstride, static_cast<float *>(h->d_obs), h->ostride, h->n, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GYMNET_OK;
    });
}

int gymnet_vecenv_get_steps_beyond_done(gymnet_vecenv *h, int32_t *out) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!h->d_sbd) return fail(h, GYMNET_ERR_UNSUPPORTED, "steps_beyond_done exists only for CartPole without GYMNET_FLAG_AUTORESET");
    if (!out) return fail(h, GYMNET_ERR_INVALID_ARG, "out is null");
    HIP_TRY(h, hipMemcpyAsync(out, h->d_sbd, (size_t)h->n * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GYMNET_OK;
    });
}

int gymnet_vecenv_set_steps_beyond_done(gymnet_vecenv *h, const int32_t *in) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!h->d_sbd) return fail(h, GYMNET_ERR_UNSUPPORTED, "steps_beyond_done exists only for CartPole without GYMNET_FLAG_AUTORESET");
    if (!in) return fail(h, GYMNET_ERR_INVALID_ARG, "in is null");
    HIP_TRY(h, hipMemcpyAsync(h->d_sbd, in, (size_t)h->n * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GYMNET_OK;
    });
}

int gymnet_vecenv_get_tick(gymnet_vecenv *h, uint64_t *tick) {
    return guarded([&]() -> int {
    if (!h || !tick) return fail(h, GYMNET_ERR_INVALID_ARG, "null argument");
    *tick = h->tick;
    return GYMNET_OK;
    });
}

int gymnet_vecenv_set_tick(gymnet_vecenv *h, uint64_t tick) {
    return guarded([&]() -> int {
    ENTER(h);
    h->tick = tick;
    touch_epoch(h);           // whatever the value: the same tick stored again is still no step an attachment saw
    return write_tick(h);
    });
}

int gymnet_vecenv_counters(gymnet_vecenv *h, gymnet_counters *out) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!out) return fail(h, GYMNET_ERR_INVALID_ARG, "out is null");
    std::memset(out, 0, sizeof *out);
    out->struct_size = sizeof *out;
    std::vector<unsigned long long> adv((size_t)kShards * kAfterStride);
    HIP_TRY(h, hipMemcpyAsync(adv.data(), h->d_after_done, adv.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    std::vector<uint32_t> cntv;
    if (h->d_done_count2 && h->last_cparity >= 0) {
        cntv.resize((size_t)kShards * kCountStride);
        HIP_TRY(h, hipMemcpyAsync(cntv.data(), h->d_done_count2 + (size_t)h->last_cparity * kShards * kCountStride,
                                  cntv.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    unsigned long long ad = 0;
    for (int s = 0; s < kShards; ++s) ad += adv[(size_t)s * kAfterStride];
    int64_t last_done = -1;
    if (!cntv.empty()) { last_done = 0; for (int s = 0; s < kShards; ++s) last_done += cntv[(size_t)s * kCountStride]; }
    uint64_t dtick[2] = {0, 0};
    HIP_TRY(h, hipMemcpy(dtick, h->d_tick2, sizeof dtick, hipMemcpyDeviceToHost));
    out->tick = dtick[h->tslot];   // the device's own count (== host mirror h->tick)
    out->lane_steps = h->lane_steps;
    out->stepped_after_done = ad;
    out->last_done_count = last_done;
    return GYMNET_OK;
    });
}

int gymnet_vecenv_done_lanes(gymnet_vecenv *h, int32_t *lanes_out, int64_t capacity, int64_t *count) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!h->d_done_list) return fail(h, GYMNET_ERR_UNSUPPORTED, "needs GYMNET_FLAG_DONE_LIST");
    if (!count || capacity < 0 || (capacity > 0 && !lanes_out)) return fail(h, GYMNET_ERR_INVALID_ARG, "bad count/capacity/lanes_out");
    if (h->last_cparity < 0) { *count = 0; return GYMNET_OK; }
    ST_TRY(compact_done(h, h->d_done_compact, nullptr, nullptr, nullptr, h->padded, h->d_done_total));
    uint32_t c32 = 0;
    HIP_TRY(h, hipMemcpyAsync(&c32, h->d_done_total, sizeof c32, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const int64_t c = (int64_t)c32;
    *count = c;
    const int64_t m = c < capacity ? c : capacity;
    if (m > 0) HIP_TRY(h, hipMemcpy(lanes_out, h->d_done_compact, (size_t)m * 4, hipMemcpyDeviceToHost));
    return GYMNET_OK;
    });
}

int gymnet_vecenv_done_lanes_device(gymnet_vecenv *h, int32_t *d_lanes_out, uint32_t *d_count_out) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!h->d_done_list) return fail(h, GYMNET_ERR_UNSUPPORTED, "needs GYMNET_FLAG_DONE_LIST");
    if (!d_count_out) return fail(h, GYMNET_ERR_INVALID_ARG, "d_count_out is null");
    if (h->last_cparity < 0) { HIP_TRY(h, hipMemsetAsync(d_count_out, 0, sizeof(uint32_t), h->stream)); return GYMNET_OK; }
    return compact_done(h, d_lanes_out ? d_lanes_out : h->d_done_compact, nullptr, nullptr, nullptr, h->padded, d_count_out);
    });
}

int gymnet_vecenv_done_records_device(gymnet_vecenv *h, int32_t *d_lanes, float *d_return, int32_t *d_length, void *d_final_obs,
                                      int64_t capacity, uint32_t *d_count) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!h->d_done_list) return fail(h, GYMNET_ERR_UNSUPPORTED, "needs GYMNET_FLAG_DONE_LIST");
    if (capacity < 0) return fail(h, GYMNET_ERR_INVALID_ARG, "capacity < 0");
    if ((d_return || d_length) && !h->d_rec_ret) return fail(h, GYMNET_ERR_UNSUPPORTED, "episode records need GYMNET_FLAG_EPISODE_STATS");
    if (d_final_obs && !h->d_rec_obs) return fail(h, GYMNET_ERR_UNSUPPORTED, "terminal observations need GYMNET_FLAG_FINAL_OBS");
    if (h->last_cparity < 0) { if (d_count) HIP_TRY(h, hipMemsetAsync(d_count, 0, sizeof(uint32_t), h->stream)); return GYMNET_OK; }
    return compact_done(h, d_lanes, d_return, d_length, d_final_obs, capacity, d_count);
    });
}

int gymnet_vecenv_done_records(gymnet_vecenv *h, int32_t *lanes_out, float *return_out, int32_t *length_out, void *final_obs_out,
                               int64_t capacity, int64_t *count) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!h->d_done_list) return fail(h, GYMNET_ERR_UNSUPPORTED, "needs GYMNET_FLAG_DONE_LIST");
    if (!count || capacity < 0) return fail(h, GYMNET_ERR_INVALID_ARG, "bad count/capacity");
    if ((return_out || length_out) && !h->d_rec_ret) return fail(h, GYMNET_ERR_UNSUPPORTED, "episode records need GYMNET_FLAG_EPISODE_STATS");
    if (final_obs_out && !h->d_rec_obs) return fail(h, GYMNET_ERR_UNSUPPORTED, "terminal observations need GYMNET_FLAG_FINAL_OBS");
    if (h->last_cparity < 0) { *count = 0; return GYMNET_OK; }
    const int O = h->desc->obs_dim;
    if ((return_out || length_out) && !h->d_rec_ret_c) { ST_TRY(dalloc(h, &h->d_rec_ret_c, (size_t)h->padded)); ST_TRY(dalloc(h, &h->d_rec_len_c, (size_t)h->padded)); }
    if (final_obs_out && !h->d_rec_obs_c) ST_TRY(dalloc(h, (char **)&h->d_rec_obs_c, (size_t)h->padded * O * h->esz));
    ST_TRY(compact_done(h, h->d_done_compact, (return_out || length_out) ? h->d_rec_ret_c : nullptr, (return_out || length_out) ? h->d_rec_len_c : nullptr,
                        final_obs_out ? h->d_rec_obs_c : nullptr, h->padded, h->d_done_total));
    uint32_t c32 = 0;
    HIP_TRY(h, hipMemcpyAsync(&c32, h->d_done_total, sizeof c32, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *count = (int64_t)c32;
    const size_t m = (size_t)((int64_t)c32 < capacity ? (int64_t)c32 : capacity);
    if (m > 0) {
        if (lanes_out) HIP_TRY(h, hipMemcpyAsync(lanes_out, h->d_done_compact, m * 4, hipMemcpyDeviceToHost, h->stream));
        if (return_out) HIP_TRY(h, hipMemcpyAsync(return_out, h->d_rec_ret_c, m * 4, hipMemcpyDeviceToHost, h->stream));
        if (length_out) HIP_TRY(h, hipMemcpyAsync(length_out, h->d_rec_len_c, m * 4, hipMemcpyDeviceToHost, h->stream));
        if (final_obs_out) HIP_TRY(h, hipMemcpyAsync(final_obs_out, h->d_rec_obs_c, m * O * h->esz, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return GYMNET_OK;
    });
}

int gymnet_vecenv_episode_stats(gymnet_vecenv *h, float *finished_return, int32_t *finished_length) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!h->d_fin_ret) return fail(h, GYMNET_ERR_UNSUPPORTED, "needs GYMNET_FLAG_EPISODE_STATS");
    // GYMNET_FLAG_COMPACT_RECORDS_ONLY: the step wrote compact records only — bring the dense view up to date for the most recent step
    if (h->compact_only && h->d_rec_ret && h->last_cparity >= 0) ST_TRY(compact_done(h, nullptr, nullptr, nullptr, nullptr, 0, nullptr, true));
    if (finished_return) HIP_TRY(h, hipMemcpyAsync(finished_return, h->d_fin_ret, (size_t)h->n * 4, hipMemcpyDeviceToHost, h->stream));
    if (finished_length) HIP_TRY(h, hipMemcpyAsync(finished_length, h->d_fin_len, (size_t)h->n * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GYMNET_OK;
    });
}

int gymnet_vecenv_final_obs(gymnet_vecenv *h, void *final_obs_out) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!h->d_final_obs) return fail(h, GYMNET_ERR_UNSUPPORTED, "needs GYMNET_FLAG_FINAL_OBS");
    if (!final_obs_out) return fail(h, GYMNET_ERR_INVALID_ARG, "final_obs_out is null");
    if (h->compact_only && h->d_rec_obs && h->last_cparity >= 0) ST_TRY(compact_done(h, nullptr, nullptr, nullptr, nullptr, 0, nullptr, true));
    ST_TRY(ensure_staging(h, false, true, false));
    HIP_TRY(h, pack_current_obs(h, h->d_final_obs, h->n, h->d_pack));       // dense terminal observations [O][n] -> row-major
    HIP_TRY(h, hipMemcpyAsync(final_obs_out, h->d_pack, (size_t)h->n * h->desc->obs_dim * h->esz, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GYMNET_OK;
    });
}

int gymnet_sample_discrete_device(int device, void *stream, int32_t *d_out, int64_t count, int32_t n, int32_t start,
                                  uint64_t seed, uint64_t lane_offset, uint64_t tick) {
    return guarded([&]() -> int {
    if (!d_out || count < 0 || n <= 0) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "bad d_out/count/n");
    DeviceScope dev_scope;
    HIP_TRY(nullptr, hipSetDevice(device));
    HIP_TRY(nullptr, launch_sample_discrete(d_out, count, n, start, seed, lane_offset, tick, static_cast<hipStream_t>(stream)));
    return GYMNET_OK;
    });
}

int gymnet_sample_discrete_masked_device(int device, void *stream, int32_t *d_out, int64_t count, int32_t n, int32_t start,
                                         const uint8_t *d_mask, int64_t mask_stride, uint64_t seed, uint64_t lane_offset, uint64_t tick) {
    return guarded([&]() -> int {
    if (!d_out || count < 0 || n <= 0) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "bad d_out/count/n");
    if (!d_mask) return gymnet_sample_discrete_device(device, stream, d_out, count, n, start, seed, lane_offset, tick);   // Discrete.cs:27
    if (mask_stride != 0 && mask_stride < n) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "mask_stride must be 0 (shared row) or >= n");
    DeviceScope dev_scope;
    HIP_TRY(nullptr, hipSetDevice(device));
    HIP_TRY(nullptr, launch_sample_discrete_masked(d_out, count, n, start, d_mask, mask_stride, seed, lane_offset, tick, static_cast<hipStream_t>(stream)));
    return GYMNET_OK;
    });
}

int gymnet_vecenv_sample_actions_masked_device(gymnet_vecenv *h, int32_t *d_actions, const uint8_t *d_mask, int64_t mask_stride,
                                               uint64_t seed, uint64_t tick) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!d_actions) return fail(h, GYMNET_ERR_INVALID_ARG, "d_actions is null");
    const EnvDesc &d = *h->desc;
    if (d.box_action) return fail(h, GYMNET_ERR_UNSUPPORTED, "Box.sample cannot be provided a mask.");   // Box.cs:70
    if (d_mask && mask_stride != 0 && mask_stride < d.action_n) return fail(h, GYMNET_ERR_INVALID_ARG, "mask_stride must be 0 (shared row) or >= n");
    if (!d_mask)
        HIP_TRY(h, launch_sample_discrete(d_actions, h->n, d.action_n, 0, seed, (uint64_t)h->cfg.lane_offset, tick, h->stream));
    else
        HIP_TRY(h, launch_sample_discrete_masked(d_actions, h->n, d.action_n, 0, d_mask, mask_stride, seed,
                                                 (uint64_t)h->cfg.lane_offset, tick, h->stream));
    return GYMNET_OK;
    });
}

int gymnet_sample_box_device(int device, void *stream, float *d_out, int64_t count, float low, float high,
                             uint64_t seed, uint64_t lane_offset, uint64_t tick) {
    return guarded([&]() -> int {
    if (!d_out || count < 0 || !(low <= high)) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "bad d_out/count/bounds");
    DeviceScope dev_scope;
    HIP_TRY(nullptr, hipSetDevice(device));
    HIP_TRY(nullptr, launch_sample_box(d_out, count, low, high, seed, lane_offset, tick, static_cast<hipStream_t>(stream)));
    return GYMNET_OK;
    });
}

int gymnet_sample_box_elementwise_device(int device, void *stream, float *d_out, int64_t count, int32_t dim, const float *d_low,
                                         const float *d_high, uint64_t seed, uint64_t lane_offset, uint64_t tick) {
    return guarded([&]() -> int {
    if (!d_out || !d_low || !d_high || count < 0 || dim <= 0) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "bad d_out/d_low/d_high/count/dim");
    DeviceScope dev_scope;
    HIP_TRY(nullptr, hipSetDevice(device));
    HIP_TRY(nullptr, launch_sample_box_elementwise(d_out, count, dim, d_low, d_high, seed, lane_offset, tick, static_cast<hipStream_t>(stream)));
    return GYMNET_OK;
    });
}

int gymnet_vecenv_sample_actions_device(gymnet_vecenv *h, void *d_actions, uint64_t seed, uint64_t tick) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!d_actions) return fail(h, GYMNET_ERR_INVALID_ARG, "d_actions is null");
    const EnvDesc &d = *h->desc;
    if (d.box_action)
        HIP_TRY(h, launch_sample_box(static_cast<float *>(d_actions), h->n, d.action_low, d.action_high, seed,
                                     (uint64_t)h->cfg.lane_offset, tick, h->stream));
    else
        HIP_TRY(h, launch_sample_discrete(static_cast<int32_t *>(d_actions), h->n, d.action_n, 0, seed,
                                          (uint64_t)h->cfg.lane_offset, tick, h->stream));
    return GYMNET_OK;
    });
}

int gymnet_vecenv_compose_actions_device(gymnet_vecenv *h, const int32_t *d_policy_actions, float epsilon, int32_t *d_actions_out,
                                         uint64_t seed, uint64_t tick) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!d_policy_actions || !d_actions_out) return fail(h, GYMNET_ERR_INVALID_ARG, "null action buffer");
    if (h->desc->box_action) return fail(h, GYMNET_ERR_UNSUPPORTED, "epsilon-greedy composition is defined for Discrete action spaces");
    if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return fail(h, GYMNET_ERR_INVALID_ARG, "epsilon must be in [0, 1]");
    HIP_TRY(h, launch_compose_discrete(d_policy_actions, d_actions_out, h->n, h->desc->action_n, epsilon, seed,
                                       (uint64_t)h->cfg.lane_offset, tick, h->stream));
    return GYMNET_OK;
    });
}

int gymnet_vecenv_sample_actions(gymnet_vecenv *h, void *actions_out, uint64_t seed, uint64_t tick) {
    return guarded([&]() -> int {
    if (!h) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "null handle");
    if (!actions_out) return fail(h, GYMNET_ERR_INVALID_ARG, "actions_out is null");
    {
        ENTER(h);
        ST_TRY(ensure_staging(h, true, false, false));
    }
    ST_TRY(gymnet_vecenv_sample_actions_device(h, h->d_actions, seed, tick));
    ENTER(h);
    HIP_TRY(h, hipMemcpyAsync(actions_out, h->d_actions, (size_t)h->n * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GYMNET_OK;
    });
}

int gymnet_vecenv_get_seed(gymnet_vecenv *h, uint64_t *seed, int32_t *per_lane) {
    return guarded([&]() -> int {
    if (!h) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "null handle");
    if (seed) *seed = h->seed;
    if (per_lane) *per_lane = h->d_lane_seed ? 1 : 0;
    return GYMNET_OK;
    });
}

}  // extern "C"

namespace {
// the per-lane array behind a gymnet_array_id: device pointer, bytes, row stride / rows for the one 2-D member
struct ArrayRef { void *p; size_t row_bytes; int rows; size_t pitch; const char *needs; };
ArrayRef array_ref(gymnet_vecenv *h, int which) {
    const size_t n = (size_t)h->n;
    switch (which) {
        case GYMNET_ARRAY_REWARD: return {h->d_reward, n * 4, 1, 0, nullptr};
        case GYMNET_ARRAY_DONE: return {h->d_done, n, 1, 0, nullptr};
        case GYMNET_ARRAY_STEPS_BEYOND_DONE: return {h->d_sbd, n * 4, 1, 0, "CartPole without GYMNET_FLAG_AUTORESET"};
        case GYMNET_ARRAY_EPISODE_RETURN: return {h->d_ep_ret, n * 4, 1, 0, "GYMNET_FLAG_EPISODE_STATS"};
        case GYMNET_ARRAY_EPISODE_LENGTH: return {h->d_ep_len, n * 4, 1, 0, "GYMNET_FLAG_EPISODE_STATS"};
        case GYMNET_ARRAY_FINISHED_RETURN: return {h->d_fin_ret, n * 4, 1, 0, "GYMNET_FLAG_EPISODE_STATS"};
        case GYMNET_ARRAY_FINISHED_LENGTH: return {h->d_fin_len, n * 4, 1, 0, "GYMNET_FLAG_EPISODE_STATS"};
        case GYMNET_ARRAY_FINAL_OBS: return {h->d_final_obs, n * h->esz, h->desc->obs_dim, n * h->esz, "GYMNET_FLAG_FINAL_OBS"};
        case GYMNET_ARRAY_LANE_SEEDS: return {h->d_lane_seed, n * 8, 1, 0, "per-lane seeds (gymnet_vecenv_seed_lanes)"};
        default: return {nullptr, 0, 0, 0, "a gymnet_array_id"};
    }
}
}  // namespace

extern "C" {

int gymnet_vecenv_get_array(gymnet_vecenv *h, int32_t which, void *out, int64_t bytes) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!out) return fail(h, GYMNET_ERR_INVALID_ARG, "out is null");
    // with compact records only, the dense "last finished episode" arrays are brought up to date first (as their getters do)
    if (h->compact_only && h->last_cparity >= 0 &&
        (((which == GYMNET_ARRAY_FINISHED_RETURN || which == GYMNET_ARRAY_FINISHED_LENGTH) && h->d_rec_ret) || (which == GYMNET_ARRAY_FINAL_OBS && h->d_rec_obs)))
        ST_TRY(compact_done(h, nullptr, nullptr, nullptr, nullptr, 0, nullptr, true));
    const ArrayRef a = array_ref(h, which);
    if (!a.p) return fail(h, which < 0 || which > GYMNET_ARRAY_LANE_SEEDS ? GYMNET_ERR_INVALID_ARG : GYMNET_ERR_UNSUPPORTED, "array %d needs %s", which, a.needs);
    if (bytes != (int64_t)(a.row_bytes * a.rows)) return fail(h, GYMNET_ERR_INVALID_ARG, "array %d holds %zu bytes, caller passed %lld", which, a.row_bytes * a.rows, (long long)bytes);
    HIP_TRY(h, hipMemcpyAsync(out, a.p, a.row_bytes * a.rows, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GYMNET_OK;
    });
}

int gymnet_vecenv_set_array(gymnet_vecenv *h, int32_t which, const void *in, int64_t bytes) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!in) return fail(h, GYMNET_ERR_INVALID_ARG, "in is null");
    if (which == GYMNET_ARRAY_LANE_SEEDS && !h->d_lane_seed) {
        // installs per-lane keys WITHOUT touching the engine tick (gymnet_vecenv_seed_lanes rewinds it): checkpoint restore
        if (bytes != h->n * 8) return fail(h, GYMNET_ERR_INVALID_ARG, "array %d holds %lld bytes, caller passed %lld", which, (long long)h->n * 8, (long long)bytes);
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (!h->d_lane_seed_buf) ST_TRY(dalloc(h, &h->d_lane_seed_buf, (size_t)h->n));
        h->d_lane_seed = h->d_lane_seed_buf;
        recompute_extras(h);
        drop_graphs(h);
    }
    const ArrayRef a = array_ref(h, which);
    if (!a.p) return fail(h, which < 0 || which > GYMNET_ARRAY_LANE_SEEDS ? GYMNET_ERR_INVALID_ARG : GYMNET_ERR_UNSUPPORTED, "array %d needs %s", which, a.needs);
    if (bytes != (int64_t)(a.row_bytes * a.rows)) return fail(h, GYMNET_ERR_INVALID_ARG, "array %d holds %zu bytes, caller passed %lld", which, a.row_bytes * a.rows, (long long)bytes);
    HIP_TRY(h, hipMemcpyAsync(a.p, in, a.row_bytes * a.rows, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    // the compacted done list / records describe the step that produced the PREVIOUS flags: not part of a restored state
    if (which == GYMNET_ARRAY_DONE) h->last_cparity = -1;
    if (which == GYMNET_ARRAY_LANE_SEEDS) touch_epoch(h);   // new keys: what seed_lanes does, less the tick
    return GYMNET_OK;
    });
}

}  // extern "C"
