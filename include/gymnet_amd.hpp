// gymnet_amd.hpp — header-only C++17 host mirror of the reference interface for this path, over the C ABI
// (gymnet_amd.h).  The reference is compiled C#; with no .NET toolchain in the build image this is the
// compiled-language host side: same member names, argument meaning and error behaviour as
//   VecEnv / IVecEnv   src/Gym/Envs/VecEnv.cs:12-93, src/Gym/Envs/IVecEnv.cs:8-19
//   Env / IEnv         src/Gym/Envs/Env.cs:13-41
//   Space/Box/Discrete src/Gym/Spaces/{Space.cs:5-18,Box.cs:15-96,Discrete.cs:5-44}
//   Step               src/Gym/Observations/Step.cs:7-29
//   exceptions         src/Gym/Exceptions/*.cs
// (paths relative to the Gym.NET tree).  NDArray is std::vector<float> here (row-major [N, D]).
// Nothing in this header computes: every call lands in libgymnet_amd.so's HIP kernels.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "gymnet_amd.h"

namespace gymnet {

// ---- exceptions (src/Gym/Exceptions) ---------------------------------------------------------------------
struct GymNetError : std::runtime_error { using std::runtime_error::runtime_error; };
struct NoDeviceError : GymNetError { using GymNetError::GymNetError; };
struct InvalidActionError : std::runtime_error {            // InvalidActionError.cs:7-10
    explicit InvalidActionError(const std::string &m = "Action is outside of the configured action space.") : std::runtime_error(m) {}
};
struct AlreadySteppingError : std::runtime_error {          // AlreadySteppingError.cs:8-10
    AlreadySteppingError() : std::runtime_error("already running an async step") {}
};
struct NotSteppingError : std::runtime_error {              // NotSteppingError.cs:4-6
    NotSteppingError() : std::runtime_error("not running an async step") {}
};

/// status -> the exception the reference throws for the same condition
inline void check(int status) {
    if (status == GYMNET_OK) return;
    const char *m = gymnet_last_error();
    std::string msg = (m && *m) ? m : gymnet_status_string(status);
    switch (status) {
        case GYMNET_ERR_INVALID_ARG: throw std::invalid_argument(msg);          // ArgumentException (VecEnv.cs:49)
        case GYMNET_ERR_INVALID_ACTION: throw InvalidActionError(msg);
        case GYMNET_ERR_ALREADY_STEPPING: throw AlreadySteppingError();
        case GYMNET_ERR_NOT_STEPPING: throw NotSteppingError();
        case GYMNET_ERR_NO_DEVICE: throw NoDeviceError(msg);
        case GYMNET_ERR_OOM: throw std::bad_alloc();
        case GYMNET_ERR_UNSUPPORTED: throw std::logic_error(msg);               // NotSupportedException
        default: throw GymNetError(msg + " (gymnet status " + std::to_string(status) + ")");
    }
}

// ---- spaces ----------------------------------------------------------------------------------------------
class Space {                                                // Space.cs:5-18
public:
    std::vector<int64_t> Shape;
    virtual ~Space() = default;
    virtual void Seed(int seed) = 0;
};

class Discrete : public Space {                              // Discrete.cs:5-44
public:
    int N, Start;
    explicit Discrete(int n, int seed = -1, int start = 0) : N(n), Start(start), rng_(seed == -1 ? std::random_device{}() : (unsigned)seed) { Shape = {n}; }
    int Sample() { return Start + (int)(rng_() % (unsigned)N); }                // Discrete.cs:27: Start + randint(0, N)
    int Sample(const std::vector<int> &mask) {                                  // Discrete.cs:18-26
        std::vector<int> valid;
        for (int i = 0; i < (int)mask.size(); ++i) if (mask[i] == 1) valid.push_back(i);
        return valid.empty() ? Start : Start + valid[rng_() % valid.size()];
    }
    bool Contains(int x) const { return x >= 0 && x < N; }                      // Discrete.cs:38-40 (ignores Start)
    void Seed(int seed) override { rng_.seed((unsigned)seed); }
private:
    std::mt19937 rng_;
};

class Box : public Space {                                   // Box.cs:15-96
public:
    enum class BoundedManner { Both, Below, Above };         // Box.cs:9-14
    std::vector<float> Low, High;
    std::vector<bool> BoundedLow, BoundedHigh;
    Box(float low, float high, int64_t n = 1, int seed = -1) : Box(std::vector<float>((size_t)n, low), std::vector<float>((size_t)n, high), seed) {}
    Box(std::vector<float> low, std::vector<float> high, int seed = -1)
        : Low(std::move(low)), High(std::move(high)), rng_(seed == -1 ? std::random_device{}() : (unsigned)seed) {
        if (Low.size() != High.size()) throw std::invalid_argument("low/high shape mismatch");
        Shape = {(int64_t)Low.size()};
        for (size_t i = 0; i < Low.size(); ++i) {                               // CheckBounded, Box.cs:49-54
            BoundedLow.push_back(Low[i] > -std::numeric_limits<float>::infinity());
            BoundedHigh.push_back(High[i] < std::numeric_limits<float>::infinity());
        }
    }
    bool IsBounded(BoundedManner manner = BoundedManner::Both) const {          // Box.cs:56-70
        bool below = true, above = true;
        for (size_t i = 0; i < Low.size(); ++i) { below = below && BoundedLow[i]; above = above && BoundedHigh[i]; }
        return manner == BoundedManner::Both ? (below && above) : manner == BoundedManner::Above ? above : below;
    }
    std::vector<float> Sample() {                                               // Box.cs:72-93, the reference's four regimes
        std::vector<float> s(Low.size());
        for (size_t i = 0; i < s.size(); ++i) {
            if (BoundedLow[i] && BoundedHigh[i]) {
                // High - Low overflows float for bounds as wide as CartPole's +-float.MaxValue velocities (CartPoleEnv.cs:46-48), and
                // uniform_real_distribution then returns inf / NaN: draw those as Low * (1 - u) + High * u, which cannot overflow
                if (std::isfinite(High[i] - Low[i])) s[i] = std::uniform_real_distribution<float>(Low[i], High[i])(rng_);
                else { const float u = std::uniform_real_distribution<float>(0.0f, 1.0f)(rng_); s[i] = Low[i] * (1.0f - u) + High[i] * u; }
            } else if (BoundedLow[i]) s[i] = std::exponential_distribution<float>(1.0f)(rng_) + Low[i];
            else if (BoundedHigh[i]) s[i] = std::exponential_distribution<float>(1.0f)(rng_) + High[i];   // sic, Box.cs:84
            else s[i] = std::normal_distribution<float>(0.5f, 1.0f)(rng_);                                // sic, Box.cs:82
        }
        return s;
    }
    bool Contains(const std::vector<float> &x) const {                          // Box.cs:95-99
        if (x.size() != Low.size()) return false;
        for (size_t i = 0; i < x.size(); ++i) if (!(x[i] >= Low[i] && x[i] <= High[i])) return false;
        return true;
    }
    void Seed(int seed) override { rng_.seed((unsigned)seed); }
private:
    std::mt19937 rng_;
};

// ---- Step records ------------------------------------------------------------------------------------------
struct Step {                                                // Step.cs:7-20; Information is always null on this path
    std::vector<float> Observation;
    float Reward = 0.0f;
    bool Done = false;
};

/// Step[] (IVecEnv.cs:15) as three arrays; operator[] materialises the reference's per-env record.
struct BatchStep {
    std::vector<float> Observation;      // row-major [N, D]
    std::vector<float> Reward;           // [N]
    std::vector<uint8_t> Done;           // [N]
    int64_t N = 0;
    int D = 0;
    Step operator[](int64_t i) const {
        Step s;
        s.Observation.assign(Observation.begin() + i * D, Observation.begin() + (i + 1) * D);
        s.Reward = Reward[(size_t)i];
        s.Done = Done[(size_t)i] != 0;
        return s;
    }
    int64_t size() const { return N; }
};

// ---- VectorEnv : VecEnv ------------------------------------------------------------------------------------
class VectorEnv {
public:
    VectorEnv(gymnet_env_id env, int64_t num_envs, int device = 0, uint64_t seed = 0, uint32_t flags = 0,
              int64_t lane_offset = 0, void *stream = nullptr) {
        // this class hands the library std::vector<float> observation buffers: a float64 handle (8 bytes per element) would overrun
        // them, so the flag is refused HERE; CartPoleEnv64 below is the float64 host class
        if (flags & GYMNET_FLAG_F64) throw std::logic_error("gymnet::VectorEnv is the float32 host class; GYMNET_FLAG_F64 handles: use gymnet::CartPoleEnv64 or the C ABI");
        check(gymnet_env_describe((int)env, &info_));
        // everything that can throw is built BEFORE the native handle exists: a constructor that throws runs no
        // destructor, so an allocation failing after gymnet_vecenv_create would leak the handle
        if (info_.action_is_box) action_box_ = std::make_unique<Box>(info_.action_low, info_.action_high, 1);
        else action_discrete_ = std::make_unique<Discrete>(info_.action_n);
        observation_space_ = std::make_unique<Box>(std::vector<float>(info_.obs_low, info_.obs_low + info_.obs_dim),
                                                   std::vector<float>(info_.obs_high, info_.obs_high + info_.obs_dim));
        gymnet_config cfg{};
        cfg.struct_size = sizeof cfg; cfg.env_id = (int)env; cfg.num_envs = num_envs; cfg.lane_offset = lane_offset;
        cfg.device = device; cfg.flags = flags; cfg.seed = seed; cfg.stream = stream;
        n_ = num_envs; device_ = device;
        check(gymnet_vecenv_create(&cfg, &h_));
    }
    VectorEnv(const VectorEnv &) = delete;
    VectorEnv &operator=(const VectorEnv &) = delete;
    ~VectorEnv() { Close(); }

    int64_t NumberOfEnvironments() const { return n_; }                         // VecEnv.cs:24
    int ObsDim() const { return info_.obs_dim; }
    int StateDim() const { return info_.state_dim; }
    Discrete *ActionSpaceDiscrete() const { return action_discrete_.get(); }    // CartPoleEnv.cs:47
    Box *ActionSpaceBox() const { return action_box_.get(); }
    const Box &ObservationSpace() const { return *observation_space_; }         // CartPoleEnv.cs:48
    std::pair<float, float> RewardRange() const { return {info_.reward_low, info_.reward_high}; }

    void Close() {                                                              // VecEnvWrapper.cs:26-30
        if (h_) { gymnet_vecenv_destroy(h_); h_ = nullptr; }
    }
    void Seed(uint64_t seed) { check(gymnet_vecenv_seed(h_, seed)); }           // VecEnv.cs:44-46
    void Seed(const std::vector<int> &seeds) {                                  // VecEnv.cs:48-53
        std::vector<uint64_t> s(seeds.begin(), seeds.end());
        check(gymnet_vecenv_seed_lanes(h_, s.data(), (int64_t)s.size()));
    }

    std::vector<float> Reset() {                                                // VecEnvWrapper.cs:18-20
        std::vector<float> obs((size_t)n_ * info_.obs_dim);
        check(gymnet_vecenv_reset(h_, obs.data()));
        return obs;
    }
    std::vector<float> ResetWhere(const std::vector<uint8_t> *mask = nullptr) { // README.md:36-40, batched
        if (mask && (int64_t)mask->size() != n_) throw std::invalid_argument("mask length must equal NumberOfEnvironments");
        std::vector<float> obs((size_t)n_ * info_.obs_dim);
        check(gymnet_vecenv_reset_where(h_, mask ? mask->data() : nullptr, obs.data()));
        return obs;
    }
    BatchStep Step(int action) {                                                // IVecEnv.Step(int), VecEnvWrapper.cs:22-24
        BatchStep b = make_batch();
        check(gymnet_vecenv_step_broadcast(h_, action, b.Observation.data(), b.Reward.data(), b.Done.data()));
        return b;
    }
    BatchStep Step(const std::vector<int32_t> &actions) {                       // extension: one action per lane
        if ((int64_t)actions.size() != n_) throw std::invalid_argument("Number of actions passed should be equals to number of environments");
        BatchStep b = make_batch();
        check(gymnet_vecenv_step(h_, actions.data(), b.Observation.data(), b.Reward.data(), b.Done.data()));
        return b;
    }
    BatchStep Step(const std::vector<float> &actions) {                         // Box actions
        if ((int64_t)actions.size() != n_) throw std::invalid_argument("Number of actions passed should be equals to number of environments");
        BatchStep b = make_batch();
        check(gymnet_vecenv_step(h_, actions.data(), b.Observation.data(), b.Reward.data(), b.Done.data()));
        return b;
    }
    void StepAsync(const std::vector<int32_t> &actions) {                       // VecEnv.cs:63-65
        if ((int64_t)actions.size() != n_) throw std::invalid_argument("Number of actions passed should be equals to number of environments");
        check(gymnet_vecenv_step_async(h_, actions.data()));
    }
    BatchStep StepWait() {
        BatchStep b = make_batch();
        check(gymnet_vecenv_step_wait(h_, b.Observation.data(), b.Reward.data(), b.Done.data()));
        return b;
    }

    std::vector<float> GetState() const {                                       // SoA [state_dim][N]
        std::vector<float> s((size_t)n_ * info_.state_dim);
        check(gymnet_vecenv_get_state(h_, s.data()));
        return s;
    }
    void SetState(const std::vector<float> &soa) {
        if ((int64_t)soa.size() != n_ * info_.state_dim) throw std::invalid_argument("state must hold state_dim * N floats");
        check(gymnet_vecenv_set_state(h_, soa.data()));
    }
    std::vector<int32_t> GetStepsBeyondDone() const {                           // CartPoleEnv.cs:41 per lane
        std::vector<int32_t> b((size_t)n_);
        check(gymnet_vecenv_get_steps_beyond_done(h_, b.data()));
        return b;
    }
    gymnet_counters Counters() const { gymnet_counters c{}; check(gymnet_vecenv_counters(h_, &c)); return c; }

    // ---- ABI 3 ------------------------------------------------------------------------------------------------------
    /// The kernel instantiation the next step launch runs, as the launcher itself resolves it.
    std::string KernelName() const { char buf[128] = {0}; check(gymnet_vecenv_kernel_name(h_, buf, (int32_t)sizeof buf)); return buf; }
    /// Library-owned page-locked, device-mapped host buffers (valid until Close): stepping THROUGH them needs no staging copies.
    struct PinnedBuffers { void *actions; float *obs; float *reward; uint8_t *done; };
    PinnedBuffers HostBuffers() {
        PinnedBuffers b{};
        void *obs = nullptr;                                                    // typed by the handle; this class creates float32 handles
        check(gymnet_vecenv_host_buffers(h_, &b.actions, &obs, &b.reward, &b.done));
        b.obs = static_cast<float *>(obs);
        return b;
    }
    // ---- ABI 4 ------------------------------------------------------------------------------------------------------
    /// Override fields of the step kernel's launch configuration (-1 = keep); every configuration is bit-identical.
    void SetLaunchPolicy(gymnet_launch_policy p) { p.struct_size = sizeof p; check(gymnet_vecenv_set_launch_policy(h_, &p)); }
    static gymnet_launch_policy KeepPolicy() { gymnet_launch_policy p; p.struct_size = sizeof p; p.vec = p.block = p.nt = p.sequential_lanes = p.reset_form = p.lds_pipe = p.occupancy_lds_bytes = p.graph = -1; return p; }
    gymnet_launch_policy GetLaunchPolicy() const { gymnet_launch_policy p{}; check(gymnet_vecenv_get_launch_policy(h_, &p)); return p; }
    /// Any per-lane array by id (checkpoint / resume of every configuration): T must be the array's element type.
    template <class T> std::vector<T> GetArray(gymnet_array_id which, size_t count) const {
        std::vector<T> a(count);
        check(gymnet_vecenv_get_array(h_, (int32_t)which, a.data(), (int64_t)(count * sizeof(T))));
        return a;
    }
    template <class T> void SetArray(gymnet_array_id which, const std::vector<T> &a) { check(gymnet_vecenv_set_array(h_, (int32_t)which, a.data(), (int64_t)(a.size() * sizeof(T)))); }
    /// gymnet_vecenv_step with caller-owned buffers (nothing is allocated): the pinned ones above, or any host memory.
    void StepInto(const void *actions, float *obs_out, float *reward_out, uint8_t *done_out) { check(gymnet_vecenv_step(h_, actions, obs_out, reward_out, done_out)); }
    /// Compact records of the lanes that finished in the most recent step (DONE_LIST [+ EPISODE_STATS] [+ FINAL_OBS]).
    struct DoneRecordSet { std::vector<int32_t> lanes; std::vector<float> episode_return; std::vector<int32_t> episode_length; std::vector<float> final_obs; };
    DoneRecordSet DoneRecords(bool episode, bool final_obs) {
        DoneRecordSet r;
        r.lanes.resize((size_t)n_);
        if (episode) { r.episode_return.resize((size_t)n_); r.episode_length.resize((size_t)n_); }
        if (final_obs) r.final_obs.resize((size_t)n_ * info_.obs_dim);
        int64_t c = 0;
        check(gymnet_vecenv_done_records(h_, r.lanes.data(), episode ? r.episode_return.data() : nullptr, episode ? r.episode_length.data() : nullptr,
                                         final_obs ? r.final_obs.data() : nullptr, n_, &c));
        r.lanes.resize((size_t)c);
        if (episode) { r.episode_return.resize((size_t)c); r.episode_length.resize((size_t)c); }
        if (final_obs) r.final_obs.resize((size_t)c * info_.obs_dim);
        return r;
    }

    // device-resident path
    void ResetDevice() { check(gymnet_vecenv_reset_device(h_)); }
    void StepDevice(const void *d_actions) { check(gymnet_vecenv_step_device(h_, d_actions)); }
    // Frame skip (gymnet_vecenv_step_repeat_device): one DECISION — d_actions held for repeat + 1 env steps in one launch; a lane that
    // finishes inside it keeps that done byte and idles for the rest; the reward is the sum of the sub-steps taken.  repeat in [0, 255].
    void StepRepeatDevice(const void *d_actions, int32_t repeat) { check(gymnet_vecenv_step_repeat_device(h_, d_actions, repeat)); }
    /// the host-boundary form with caller-owned buffers, as StepInto
    void StepRepeatInto(const void *actions, int32_t repeat, void *obs_out, float *reward_out, uint8_t *done_out) {
        check(gymnet_vecenv_step_repeat(h_, actions, repeat, obs_out, reward_out, done_out));
    }
    /// the fused form: spec.steps DECISIONS of repeat + 1 env steps each, rec_* buffers and record indices per decision
    void RolloutRepeatDevice(gymnet_rollout_spec spec, int32_t repeat) {
        spec.struct_size = (uint32_t)sizeof spec;
        check(gymnet_vecenv_rollout_repeat_device(h_, &spec, repeat));
    }
    void RolloutDevice(const void *d_actions, int64_t steps, int64_t stride, int64_t ring) { check(gymnet_vecenv_rollout_device(h_, d_actions, steps, stride, ring)); }
    void Sync() { check(gymnet_vecenv_sync(h_)); }
    gymnet_device_view DeviceView() const { gymnet_device_view v{}; check(gymnet_vecenv_device_view(h_, &v)); return v; }
    // CartPole pixel frame stacks (gymnet_vecenv_pixel_stack_config): the Images runner's frame queue and input on the device.  The
    // defaults are its shape: two 40 x 20 frames of the crop (200, 150, 200, 150), oldest first, 1.0f where a pixel is not background.
    void ConfigurePixelStack(int32_t format = GYMNET_STACK_BINARY_F32, int32_t depth = 2, int32_t out_w = 40, int32_t out_h = 20,
                             int32_t crop_x = 200, int32_t crop_y = 150, int32_t crop_w = 200, int32_t crop_h = 150,
                             void *d_ext = nullptr, int64_t lane_stride = 0) {
        check(gymnet_vecenv_pixel_stack_config(h_, format, depth, crop_x, crop_y, crop_w, crop_h, out_w, out_h, d_ext, lane_stride));
        stack_depth_ = depth;
    }
    void ResetPixelStack(const uint8_t *d_mask = nullptr) { check(gymnet_vecenv_pixel_stack_reset_device(h_, d_mask)); }
    void PushPixelStack(const uint8_t *d_done = nullptr) { check(gymnet_vecenv_pixel_stack_push_device(h_, d_done)); }
    struct PixelStackView { void *d_stack; int64_t lane_stride, frame_bytes; };
    PixelStackView PixelStack() const { PixelStackView v{}; check(gymnet_vecenv_pixel_stack_view(h_, &v.d_stack, &v.lane_stride, &v.frame_bytes)); return v; }
    /// the stacks of lanes [first, first + count) (count < 0: to the last lane), packed [count][depth][out_h][out_w]: T = uint8_t for
    /// GRAY8 / BINARY8 stacks, float for BINARY_F32
    template <class T> std::vector<T> ReadPixelStack(int64_t first = 0, int64_t count = -1) const {
        if (count < 0) count = n_ - first;
        const PixelStackView v = PixelStack();
        if (v.frame_bytes % (int64_t)sizeof(T) != 0) throw std::invalid_argument("element type does not match the stack's format");
        std::vector<T> out((size_t)(count > 0 ? count * stack_depth_ * v.frame_bytes / (int64_t)sizeof(T) : 0));
        check(gymnet_vecenv_pixel_stack_read(h_, out.data(), first, count));
        return out;
    }
    // The episode memory (gymnet_vecenv_memory_config): every step of each lane's open episode, the best `capacity` finished episodes
    // by (return, end tick, lane) and the dataset built from them.  max_length 0 = the handle's max_episode_steps.
    void ConfigureEpisodeMemory(int32_t capacity = 100, int32_t max_length = 0, int32_t history = 4) {
        check(gymnet_vecenv_memory_config(h_, capacity, max_length, history));
    }
    /// ConfigureEpisodeMemory sized for PushMemoryRollout passes of rollout_chunk (1 .. 64) steps: rollout_chunk - 1 more staging slots and
    /// candidate segments
    void ConfigureEpisodeMemoryRollout(int32_t capacity = 100, int32_t max_length = 0, int32_t history = 4, int32_t rollout_chunk = 16) {
        check(gymnet_vecenv_memory_config_rollout(h_, capacity, max_length, history, rollout_chunk));
    }
    /// once after ONE launch of `steps` steps (any fused rollout, or a single StepDevice with steps = 1): the rows it recorded — d_rec_obs
    /// [steps][obs_dim][N], d_rec_reward and d_rec_done [steps][N] — and its actions, step t's at row (t % ring) * action_stride of d_actions
    /// (-1: a [steps][N] record, action_stride = N and ring = steps).  The memory ends as `steps` x (StepDevice, PushEpisodeMemory) would
    /// have left it
    void PushMemoryRollout(int64_t steps, const void *d_rec_obs, const void *d_actions, const float *d_rec_reward, const uint8_t *d_rec_done,
                           int64_t action_stride = -1, int64_t ring = -1) {
        check(gymnet_vecenv_memory_push_rollout_device(h_, steps, d_rec_obs, d_actions, action_stride < 0 ? n_ : action_stride,
                                                       ring < 0 ? steps : ring, d_rec_reward, d_rec_done));
    }
    void PushEpisodeMemory(const void *d_actions, const uint8_t *d_done = nullptr) { check(gymnet_vecenv_memory_push_device(h_, d_actions, d_done)); }
    void ResetEpisodeMemory(const uint8_t *d_mask = nullptr, bool clear_pool = false) {
        check(gymnet_vecenv_memory_reset_device(h_, d_mask, clear_pool ? 1 : 0));
    }
    struct MemoryStats { int64_t kept, ended, admitted, too_long; };
    MemoryStats EpisodeMemoryStats() const {
        MemoryStats s{};
        check(gymnet_vecenv_memory_stats(h_, &s.kept, &s.ended, &s.admitted, &s.too_long));
        return s;
    }
    struct MemoryEpisodes { std::vector<float> ret; std::vector<int32_t> len; std::vector<uint64_t> end_tick; std::vector<int32_t> lane; };
    /// the kept episodes in descending key order (blocks)
    MemoryEpisodes ReadMemoryEpisodes() const {
        int64_t count = 0;
        check(gymnet_vecenv_memory_episodes(h_, nullptr, nullptr, nullptr, nullptr, 0, &count));
        MemoryEpisodes e;
        e.ret.resize((size_t)count); e.len.resize((size_t)count); e.end_tick.resize((size_t)count); e.lane.resize((size_t)count);
        check(gymnet_vecenv_memory_episodes(h_, e.ret.data(), e.len.data(), e.end_tick.data(), e.lane.data(), count, &count));
        return e;
    }
    int64_t MemoryDatasetRows() const { int64_t r = 0; check(gymnet_vecenv_memory_dataset_size(h_, &r)); return r; }
    /// DataBuilder.BuildDataset into device buffers of at least capacity_rows rows (format GYMNET_MEMORY_PARAMS or GYMNET_STACK_*);
    /// returns the rows written, or -1 while fewer than min_episodes episodes are kept
    int64_t BuildMemoryDataset(void *d_x, int32_t *d_action, float *d_onehot, int64_t capacity_rows, int64_t min_episodes,
                               int32_t format = GYMNET_MEMORY_PARAMS, int32_t out_w = 40, int32_t out_h = 20, int32_t crop_x = 200,
                               int32_t crop_y = 150, int32_t crop_w = 200, int32_t crop_h = 150) {
        if (EpisodeMemoryStats().kept < min_episodes) return -1;
        const int64_t rows = MemoryDatasetRows();
        check(gymnet_vecenv_memory_dataset_device(h_, format, crop_x, crop_y, crop_w, crop_h, out_w, out_h, d_x, d_action, d_onehot, nullptr,
                                                  capacity_rows));
        return rows < capacity_rows ? rows : capacity_rows;
    }
    // The actor (gymnet_vecenv_actor_config): a fully connected ReLU network on the device that chooses every lane's action from its
    // last `history` observations.  widths = w_0 .. w_L; weights = per layer W [out][in] row-major, then b [out].  Empty widths release it.
    void ConfigureActor(int32_t history, const std::vector<int32_t> &widths, const std::vector<float> &weights) {
        if (widths.empty()) { check(gymnet_vecenv_actor_config(h_, 0, 0, nullptr, nullptr, 0)); return; }
        check(gymnet_vecenv_actor_config(h_, history, (int32_t)widths.size() - 1, widths.data(), weights.data(), (int64_t)weights.size()));
    }
    void LoadActorWeights(const float *d_weights, int64_t count) { check(gymnet_vecenv_actor_load_device(h_, d_weights, count)); }
    void ResetActor(const uint8_t *d_mask = nullptr) { check(gymnet_vecenv_actor_reset_device(h_, d_mask)); }
    void PushActor(const uint8_t *d_done = nullptr) { check(gymnet_vecenv_actor_push_device(h_, d_done)); }
    /// every lane's action (argmax of the logits, epsilon-greedy as gymnet_vecenv_compose_actions_device composes it) into d_actions
    void ActorAct(int32_t *d_actions, float epsilon = 0.0f, uint64_t seed = 0, uint64_t tick = 0, float *d_logits = nullptr) {
        check(gymnet_vecenv_actor_act_device(h_, d_actions, d_logits, epsilon, seed, tick));
    }
    // A Discrete actor's exploration setting (gymnet_vecenv_actor_set_exploration): under SOFTMAX a lane that explores draws its action from
    // softmax(logits / temperature) instead of uniformly; ActorAct and the fused actor rollout read it.  A new actor has (UNIFORM, 1).
    void SetActorExploration(gymnet_actor_explore explore, float temperature = 1.0f) {
        check(gymnet_vecenv_actor_set_exploration(h_, (int32_t)explore, temperature));
    }
    void GetActorExploration(gymnet_actor_explore &explore, float &temperature) const {
        int32_t ex = 0;
        check(gymnet_vecenv_actor_get_exploration(h_, &ex, &temperature));
        explore = (gymnet_actor_explore)ex;
    }
    // The log-probability of the action every lane takes, under softmax(logits / the stored temperature) whatever the exploration setting
    // (gymnet_vecenv_actor_act_logp_device): d_logp float32 [N]; actions and logits are ActorAct's, bit for bit.  d_logp null: ActorAct.
    void ActorActLogp(int32_t *d_actions, float *d_logp, float epsilon = 0.0f, uint64_t seed = 0, uint64_t tick = 0, float *d_logits = nullptr) {
        check(gymnet_vecenv_actor_act_logp_device(h_, d_actions, d_logits, d_logp, epsilon, seed, tick));
    }
    // The fused rollout with action_source = GYMNET_ACTIONS_ACTOR on a Discrete actor, also recording every step's log-probability into
    // d_rec_logp float32 [T][N] (gymnet_vecenv_rollout_fused_logp_device); null: gymnet_vecenv_rollout_fused_ex_device itself.
    void RolloutFusedLogp(gymnet_rollout_spec spec, float *d_rec_logp) {
        spec.struct_size = (uint32_t)sizeof spec;
        check(gymnet_vecenv_rollout_fused_logp_device(h_, &spec, d_rec_logp));
    }
    // The critic (gymnet_vecenv_actor_critic_config): a second network of the actor's kind over the actor's input, widths w_0 = history *
    // obs_dim .. w_L = 1, whose one output is the lane's value.  Needs a configured actor of either kind; empty widths remove it;
    // ConfigureActor / ConfigureBoxActor drop it.
    void ConfigureActorCritic(const std::vector<int32_t> &widths, const std::vector<float> &weights) {
        if (widths.empty()) { check(gymnet_vecenv_actor_critic_config(h_, 0, nullptr, nullptr, 0)); return; }
        check(gymnet_vecenv_actor_critic_config(h_, (int32_t)widths.size() - 1, widths.data(), weights.data(), (int64_t)weights.size()));
    }
    void LoadActorCriticWeights(const float *d_weights, int64_t count) { check(gymnet_vecenv_actor_critic_load_device(h_, d_weights, count)); }
    /// the critic over every lane's current history into d_value float32 [N]: the last value after a rollout
    void ActorValue(float *d_value) { check(gymnet_vecenv_actor_value_device(h_, d_value)); }
    // ActorActLogp that also writes the critic's value of the input each action was chosen from into d_value float32 [N]
    // (gymnet_vecenv_actor_act_value_device): actions, logits and logp are ActorActLogp's, bit for bit.  d_value null: ActorActLogp.
    void ActorActValue(int32_t *d_actions, float *d_logp, float *d_value, float epsilon = 0.0f, uint64_t seed = 0, uint64_t tick = 0,
                       float *d_logits = nullptr) {
        check(gymnet_vecenv_actor_act_value_device(h_, d_actions, d_logits, d_logp, d_value, epsilon, seed, tick));
    }
    // RolloutFusedLogp on a Discrete actor with a critic, also recording the value before every step into d_rec_value float32 [T][N]
    // (gymnet_vecenv_rollout_fused_value_device); d_rec_logp may be null.  d_rec_value null: RolloutFusedLogp itself.
    void RolloutFusedValue(gymnet_rollout_spec spec, float *d_rec_logp, float *d_rec_value) {
        spec.struct_size = (uint32_t)sizeof spec;
        check(gymnet_vecenv_rollout_fused_value_device(h_, &spec, d_rec_logp, d_rec_value));
    }
    // GAE(gamma, lambda) advantages and advantage + value over the rows a rollout recorded (gymnet_gae_device: the recurrence is written out
    // there), one launch on the handle's device and stream: ordered after the rollout, no synchronise.  d_reward float32 [steps][N], d_done
    // uint8 [steps][N] (the fused rollout's records); d_value float32 [steps][N] or null (every value 0), d_last_value float32 [N], d_boot
    // float32 [steps][N] (V(terminal observation) of truncated lanes) or null; d_advantage / d_return float32 [steps][N], either may be null.
    // d_advantage may be d_reward while d_return is d_value, or the other way round.
    void AdvantagesDevice(int64_t steps, const float *d_reward, const uint8_t *d_done, const float *d_value, const float *d_last_value,
                          float *d_advantage, float *d_return, float gamma = 0.99f, float lambda = 0.95f, const float *d_boot = nullptr) {
        check(gymnet_gae_device(device_, DeviceView().stream, steps, n_, n_, d_reward, d_done, d_value, d_last_value, d_boot, gamma, lambda, d_advantage, d_return));
    }
    // The actor's history as the caller's own float32 [history][obs_dim][N], oldest first (gymnet_vecenv_actor_history_device): one kernel
    // on the handle's stream.  Taken before a fused actor rollout it is the d_history0 of RolloutInputsDevice.
    void ActorHistoryDevice(float *d_out) { check(gymnet_vecenv_actor_history_device(h_, d_out, n_)); }
    // The network inputs a recorded rollout's actions were chosen from (gymnet_rollout_inputs_device: the rule is written out there), on
    // the handle's device and stream: ordered after the rollout, no synchronise.  d_rec_obs [steps][obs_dim][N] float32 (obs_f64: float64,
    // a float64 handle's records), d_rec_done uint8 [steps][N], d_history0 float32 [history][obs_dim][N].  d_rows null: d_x is float32
    // [steps][N][history * obs_dim]; else d_rows int64 [num_rows] flat indices t * N + lane and d_x is [num_rows][history * obs_dim].
    // d_history_out (optional) float32 [history][obs_dim][N]: the history after the last step, the next call's d_history0.
    void RolloutInputsDevice(int64_t steps, int32_t history, const void *d_rec_obs, const uint8_t *d_rec_done, const float *d_history0, float *d_x,
                             const int64_t *d_rows = nullptr, int64_t num_rows = 0, float *d_history_out = nullptr, bool obs_f64 = false) {
        check(gymnet_rollout_inputs_device(device_, DeviceView().stream, steps, n_, n_, info_.obs_dim, history, obs_f64 ? 1 : 0, d_rec_obs, d_rec_done, d_history0, n_, d_rows, num_rows, d_x, (int64_t)history * info_.obs_dim, d_history_out, n_));
    }
    // The Box actor (gymnet_vecenv_actor_box_config): the same network on Pendulum / MountainCarContinuous; its one output, clamped to the
    // env's bounds, is the action.  Empty widths release the actor.  LoadActorWeights / ResetActor / PushActor serve both kinds.
    void ConfigureBoxActor(int32_t history, const std::vector<int32_t> &widths, const std::vector<float> &weights) {
        if (widths.empty()) { check(gymnet_vecenv_actor_box_config(h_, 0, 0, nullptr, nullptr, 0)); return; }
        check(gymnet_vecenv_actor_box_config(h_, history, (int32_t)widths.size() - 1, widths.data(), weights.data(), (int64_t)weights.size()));
    }
    // d_actions float32 [N]; d_raw float32 [N] or null: the unclamped outputs
    void BoxActorAct(float *d_actions, float epsilon = 0.0f, uint64_t seed = 0, uint64_t tick = 0, float *d_raw = nullptr) {
        check(gymnet_vecenv_actor_box_act_device(h_, d_actions, d_raw, epsilon, seed, tick));
    }
    // A Box actor's policy (gymnet_vecenv_actor_box_set_policy): a tanh head and / or Gaussian noise of scale sigma around the greedy action
    // on the lanes that explore; BoxActorAct and the fused actor rollout read it.  A new actor has (CLAMP, SAMPLE, 0).
    void SetBoxActorPolicy(gymnet_box_head head, gymnet_box_explore explore, float sigma = 0.0f) {
        check(gymnet_vecenv_actor_box_set_policy(h_, (int32_t)head, (int32_t)explore, sigma));
    }
    void GetBoxActorPolicy(gymnet_box_head &head, gymnet_box_explore &explore, float &sigma) const {
        int32_t hd = 0, ex = 0;
        check(gymnet_vecenv_actor_box_get_policy(h_, &hd, &ex, &sigma));
        head = (gymnet_box_head)hd; explore = (gymnet_box_explore)ex;
    }
    // BoxActorAct that also writes the log-density of every lane's action under the handle's policy, sigma > 0, into d_logd float32 [N]
    // (gymnet_vecenv_actor_box_act_logd_device): log N(action; greedy, sigma^2); actions and raw outputs are BoxActorAct's, bit for bit.
    // d_logd null: BoxActorAct.
    void BoxActorActLogd(float *d_actions, float *d_logd, float epsilon = 0.0f, uint64_t seed = 0, uint64_t tick = 0, float *d_raw = nullptr) {
        check(gymnet_vecenv_actor_box_act_logd_device(h_, d_actions, d_raw, d_logd, epsilon, seed, tick));
    }
    // RolloutFused with GYMNET_ACTIONS_ACTOR on a Box actor, also recording every step's log-density into d_rec_logd and, with a critic, the
    // value before every step into d_rec_value, float32 [T][N] each (gymnet_vecenv_rollout_fused_box_logd_device); either may be null.
    // Both null: RolloutFused itself.
    void RolloutFusedBoxLogd(gymnet_rollout_spec spec, float *d_rec_logd, float *d_rec_value) {
        spec.struct_size = (uint32_t)sizeof spec;
        check(gymnet_vecenv_rollout_fused_box_logd_device(h_, &spec, d_rec_logd, d_rec_value));
    }
    // V(terminal observation) of every lane whose done byte has bit 1 set (a time limit), +0 for every other lane, into d_boot float32 [N]:
    // one row of AdvantagesDevice's d_boot (gymnet_vecenv_actor_boot_device).  After a vector step and before PushActor; needs a critic and
    // max_episode_steps > 0, and on an auto-reset handle GYMNET_FLAG_FINAL_OBS.  Changes neither the history nor what PushActor does next.
    void ActorBoot(float *d_boot) { check(gymnet_vecenv_actor_boot_device(h_, d_boot)); }
    // RolloutFusedValue / RolloutFusedBoxLogd that also record ActorBoot's row after every step into d_rec_boot float32 [T][N]
    // (gymnet_vecenv_rollout_fused_value_boot_device, _box_boot_device): needs d_rec_value; GYMNET_FLAG_FINAL_OBS is not needed.
    // d_rec_boot null: the call without it.
    void RolloutFusedValueBoot(gymnet_rollout_spec spec, float *d_rec_logp, float *d_rec_value, float *d_rec_boot) {
        spec.struct_size = (uint32_t)sizeof spec;
        check(gymnet_vecenv_rollout_fused_value_boot_device(h_, &spec, d_rec_logp, d_rec_value, d_rec_boot));
    }
    void RolloutFusedBoxBoot(gymnet_rollout_spec spec, float *d_rec_logd, float *d_rec_value, float *d_rec_boot) {
        spec.struct_size = (uint32_t)sizeof spec;
        check(gymnet_vecenv_rollout_fused_box_boot_device(h_, &spec, d_rec_logd, d_rec_value, d_rec_boot));
    }
    gymnet_vecenv *handle() const { return h_; }

private:
    BatchStep make_batch() const {
        BatchStep b;
        b.N = n_; b.D = info_.obs_dim;
        b.Observation.resize((size_t)n_ * info_.obs_dim); b.Reward.resize((size_t)n_); b.Done.resize((size_t)n_);
        return b;
    }
    gymnet_vecenv *h_ = nullptr;
    gymnet_env_info info_{};
    int64_t n_ = 0;
    int device_ = 0;                   // the handle's HIP device: what the handle-less calls (gymnet_gae_device) are given
    int32_t stack_depth_ = 0;         // of the pixel stack ConfigurePixelStack set up
    std::unique_ptr<Discrete> action_discrete_;
    std::unique_ptr<Box> action_box_, observation_space_;
};

/// ONE process driving G GPUs (gymnet_group_*): member m owns lanes [m*N/G, (m+1)*N/G); every member keeps a replica
/// [G][obs_dim][N/G] of all observations on its GPU, completed by AllGatherObs() (hand-written direct push over peer-mapped
/// memory, or RCCL).  The host-boundary Reset / Step take the whole batch in the NDArray layout, like VectorEnv.
class GroupVectorEnv {
public:
    GroupVectorEnv(gymnet_env_id env, int64_t global_num_envs, const std::vector<int32_t> &devices, uint64_t seed = 0,
                   uint32_t flags = GYMNET_FLAG_AUTORESET, gymnet_gather_mode gather = GYMNET_GATHER_DIRECT) {
        check(gymnet_env_describe((int)env, &info_));
        gymnet_group_config cfg{};
        cfg.struct_size = sizeof cfg; cfg.env_id = (int)env; cfg.global_num_envs = global_num_envs;
        cfg.num_members = (int32_t)devices.size(); cfg.flags = flags; cfg.seed = seed; cfg.devices = devices.data(); cfg.gather = gather;
        n_ = global_num_envs; g_members_ = (int)devices.size();
        check(gymnet_group_create(&cfg, &g_));
    }
    GroupVectorEnv(const GroupVectorEnv &) = delete;
    GroupVectorEnv &operator=(const GroupVectorEnv &) = delete;
    ~GroupVectorEnv() { Close(); }
    void Close() { if (g_) { gymnet_group_destroy(g_); g_ = nullptr; } }

    int64_t NumberOfEnvironments() const { return n_; }
    int NumMembers() const { return g_members_; }
    int ObsDim() const { return info_.obs_dim; }
    void Seed(uint64_t seed) { check(gymnet_group_seed(g_, seed)); }

    std::vector<float> Reset() {                                                // row-major [N, obs_dim]
        std::vector<float> obs((size_t)n_ * info_.obs_dim);
        check(gymnet_group_reset(g_, obs.data()));
        return obs;
    }
    BatchStep Step(const std::vector<int32_t> &actions) {
        if ((int64_t)actions.size() != n_) throw std::invalid_argument("Number of actions passed should be equals to number of environments");
        BatchStep b;
        b.N = n_; b.D = info_.obs_dim;
        b.Observation.resize((size_t)n_ * info_.obs_dim); b.Reward.resize((size_t)n_); b.Done.resize((size_t)n_);
        check(gymnet_group_step(g_, actions.data(), b.Observation.data(), b.Reward.data(), b.Done.data()));
        return b;
    }
    BatchStep Step(int action) { return Step(std::vector<int32_t>((size_t)n_, action)); }   // IVecEnv.Step(int): scalar broadcast

    void AllGatherObs() { check(gymnet_group_allgather_obs(g_)); }
    void WaitGather() { check(gymnet_group_wait_gather(g_)); }
    std::vector<float> ReadReplica(int member) {                               // [G][obs_dim][N/G] as member `member` holds it
        std::vector<float> r((size_t)n_ * info_.obs_dim);
        check(gymnet_group_read_replica(g_, member, r.data()));
        return r;
    }
    void Sync() { check(gymnet_group_sync(g_)); }
    gymnet_group *handle() const { return g_; }

private:
    gymnet_group *g_ = nullptr;
    gymnet_env_info info_{};
    int64_t n_ = 0;
    int g_members_ = 0;
};

/// Single-instance Env façade in the reference's OWN arithmetic (GYMNET_FLAG_F64): float64 state, float64 observations — what
/// `new CartPoleEnv().Step(a).Observation` really holds (CartPoleEnv.cs:141-166,185) — so the reference's loop
/// (README.md:32-52) sees the reference's states to the last few ulps and its exact episode lengths, free-running.
struct Step64 { std::vector<double> Observation; float Reward = 0.0f; bool Done = false; };
class CartPoleEnv64 {
public:
    explicit CartPoleEnv64(int device = 0, uint64_t seed = 0, uint32_t extra_flags = 0) {
        gymnet_config cfg{};
        cfg.struct_size = sizeof cfg; cfg.env_id = GYMNET_ENV_CARTPOLE; cfg.num_envs = 1; cfg.device = device;
        cfg.flags = GYMNET_FLAG_F64 | extra_flags; cfg.seed = seed;
        // (the resident latency path is opt-in: pass GYMNET_FLAG_RESIDENT in extra_flags — see CartPoleEnv below for when it pays)
        check(gymnet_vecenv_create(&cfg, &h_));
    }
    CartPoleEnv64(const CartPoleEnv64 &) = delete;
    CartPoleEnv64 &operator=(const CartPoleEnv64 &) = delete;
    ~CartPoleEnv64() { CloseEnvironment(); }
    std::vector<double> Reset() { std::vector<double> o(4); check(gymnet_vecenv_reset(h_, o.data())); return o; }   // CartPoleEnv.cs:63-67
    Step64 Step(int action) {                                                   // CartPoleEnv.cs:137-186
        Step64 s; s.Observation.resize(4);
        uint8_t d = 0;
        const int32_t a = action;
        check(gymnet_vecenv_step(h_, &a, s.Observation.data(), &s.Reward, &d));
        s.Done = d != 0;
        return s;
    }
    void SetState(const std::vector<double> &x) { if (x.size() != 4) throw std::invalid_argument("state must hold 4 doubles"); check(gymnet_vecenv_set_state(h_, x.data())); }
    std::vector<double> GetState() const { std::vector<double> x(4); check(gymnet_vecenv_get_state(h_, x.data())); return x; }
    void Seed(int seed) { check(gymnet_vecenv_seed(h_, (uint64_t)seed)); }      // CartPoleEnv.cs:196-198
    void CloseEnvironment() { if (h_) { gymnet_vecenv_destroy(h_); h_ = nullptr; } }   // CartPoleEnv.cs:189-194
    gymnet_vecenv *handle() const { return h_; }
private:
    gymnet_vecenv *h_ = nullptr;
};

/// Single-instance Env façade (Env.cs:13-41; CartPoleEnv.cs:43-198) over a 1-lane float32 VectorEnv (the batched engine's
/// arithmetic: 1e-5 per teacher-forced step; CartPoleEnv64 above is the reference-exact one).
class CartPoleEnv {
public:
    /// resident = true (opt-in since round 6): GYMNET_FLAG_RESIDENT — Step / Reset are served by a resident single-wave kernel through a
    /// mailbox in pinned host memory (no launch, no synchronize per call; ~3x lower latency for a loop that only steps; bit-identical).
    /// While it waits for the next command the kernel occupies the handle's stream for up to ~5 ms: a device-wide synchronize elsewhere
    /// in the process waits for that, which is why a host that also trains on the GPU keeps the default (one launch per call).
    explicit CartPoleEnv(int device = 0, uint64_t seed = 0, bool resident = false) : v_(GYMNET_ENV_CARTPOLE, 1, device, seed, resident ? GYMNET_FLAG_RESIDENT : 0u) {}
    std::vector<float> Reset() { return v_.Reset(); }                           // CartPoleEnv.cs:63-67
    gymnet::Step Step(int action) { return v_.Step(std::vector<int32_t>{action})[0]; }   // CartPoleEnv.cs:137-186
    /// Env<TAction>.Step(TAction) where TAction : Enum (Env.cs:43-53): the enum's integer value is the discrete action
    template <class TAction, std::enable_if_t<std::is_enum<TAction>::value, int> = 0>
    gymnet::Step Step(TAction action) { return Step(static_cast<int>(action)); }
    void Seed(int seed) { v_.Seed((uint64_t)seed); }                            // CartPoleEnv.cs:196-198
    void CloseEnvironment() { v_.Close(); }                                     // CartPoleEnv.cs:189-194
    Discrete &ActionSpace() { return *v_.ActionSpaceDiscrete(); }
    const Box &ObservationSpace() const { return v_.ObservationSpace(); }
    VectorEnv &vector() { return v_; }
private:
    VectorEnv v_;
};

}  // namespace gymnet
