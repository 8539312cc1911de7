// rollout_inputs.hip — the network inputs a recorded rollout's actions were chosen from: for step t of a lane the lane's last S
// observations before the step, oldest first, clamped to the episode's first one.  The contract, operation for operation, is
// gymnet_rollout_inputs_device in include/gymnet_amd.h; tests/_rollout_inputs_twin.py applies the push rule T times and the GPU tests
// compare bits.  Pure data movement: every value is a 32-bit pattern that is loaded and stored (float64 observations are rounded once).
//
// Where the values come from.  Number the observations a lane has seen by the step that produced them: j >= 0 is d_rec_obs[j], j < 0 is
// row S + j of d_history0.  With no done byte the input of step t is the observations t - S .. t - 1; a done byte on row r makes every
// slot of the history observation r, so with `last` = the newest row < t whose done byte is set, slot s of the input of step t is
//     observation max(t - S + s, last).
// Only a done byte on rows t - S + 1 .. t - 1 can exceed t - S + s: looking back stops after S - 1 done bytes, or at the first one set.
//
// The kernels hold no window in registers: obs_dim and S are run-time values, so a window would be indexed dynamically, and re-reading a
// value the same thread read one row earlier is served by the caches at a rate that is no bound — the call writes S times what it reads
// and is bound by its stores.  So the work is laid out for the stores.  One thread owns V consecutive floats of an output row and
// consecutive threads own consecutive floats: where x_row_stride == S * obs_dim the rows of neighbouring lanes are contiguous and each
// store instruction of a wave covers 64 * V * 4 contiguous bytes (1 KiB at V = 4), with no staging through LDS.  (A thread that owns a
// whole lane stores 16 bytes at a stride of a row, 64 bytes for CartPole at S = 4: GYMNET_ROLLOUT_INPUTS_LANE_MAJOR=1 builds that
// assignment for tools/rollout_inputs_probe.py to time; docs/ledger.md §rollout inputs has the numbers.)
//   dense:    a thread walks the rows t of one chunk (rollout_inputs.hpp: rows_per_chunk) carrying `last`; the done byte of row t and the
//             values of row t are loaded side by side, kRowsInFlight rows at a time, before the stores of those rows.
//   gathered: a thread looks `last` up for its row index and writes its V floats; a row index outside [0, steps * count) gives NaN.
//   history:  d_history_out = the input of "step `steps`", one thread per lane, stored [S][obs_dim][lane].
#include "rollout_inputs.hpp"
#include "handle.hpp"

#ifndef GYMNET_ROLLOUT_INPUTS_LANE_MAJOR
#define GYMNET_ROLLOUT_INPUTS_LANE_MAJOR 0
#endif
#ifndef GYMNET_ROLLOUT_INPUTS_TARGET_THREADS
#define GYMNET_ROLLOUT_INPUTS_TARGET_THREADS ::gymnet::kRolloutInputsTargetThreads
#endif

namespace gymnet {

namespace {

constexpr int64_t kNoDone = INT64_MIN / 2;        // `last` where no done byte was met: below every observation number
constexpr uint32_t kCanonicalNaN = 0x7FC00000u;
constexpr int kRowsInFlight = 4;

struct InputsArgs {
    const void *rec_obs; const uint8_t *rec_done; const uint32_t *history0; const int64_t *rows;
    uint32_t *x; uint32_t *history_out;
    int64_t steps, count, stride, history0_stride, x_row_stride, history_out_stride;
    int64_t cols, col_blocks, rows_per_chunk, per_row;
    int32_t obs_dim, history;
};

typedef uint32_t uint4v __attribute__((ext_vector_type(4)));
template <int V> struct Word;
template <> struct Word<1> { using T = uint32_t; };
template <> struct Word<4> { using T = uint4v; };
__device__ __forceinline__ void set_word(uint32_t &w, int, uint32_t v) { w = v; }
__device__ __forceinline__ void set_word(uint4v &w, int j, uint32_t v) { w[j] = v; }

// value k of observation `src` of lane i, as float32 bits
template <bool F64>
__device__ __forceinline__ uint32_t observation_bits(const InputsArgs &a, int64_t src, int32_t k, int64_t i) {
    if (src < 0) return a.history0[((a.history + src) * a.obs_dim + k) * a.history0_stride + i];
    const int64_t off = (src * a.obs_dim + k) * a.stride + i;
    if constexpr (F64) return __float_as_uint((float)static_cast<const double *>(a.rec_obs)[off]);     // round to nearest even
    else return static_cast<const uint32_t *>(a.rec_obs)[off];
}

// the newest row below t whose done byte is set, among the history - 1 rows that can matter to step t
__device__ __forceinline__ int64_t last_done_before(const InputsArgs &a, int64_t t, int64_t i) {
    const int64_t lo = t - (a.history - 1) > 0 ? t - (a.history - 1) : 0;
    for (int64_t r = t - 1; r >= lo; --r)
        if (a.rec_done[r * a.stride + i] != 0) return r;
    return kNoDone;
}

// slot and value index of each of the thread's V floats, first float e0 of the row
template <int V>
struct Slots {
    int32_t s[V], k[V];
    __device__ __forceinline__ Slots(const InputsArgs &a, int64_t e0) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int32_t e = (int32_t)e0 + v;
            s[v] = e / a.obs_dim;
            k[v] = e - s[v] * a.obs_dim;
        }
    }
};

template <int V, bool F64>
__device__ __forceinline__ typename Word<V>::T input_word(const InputsArgs &a, const Slots<V> &sl, int64_t t, int64_t last, int64_t i) {
    typename Word<V>::T w;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int64_t j = t - a.history + sl.s[v];
        set_word(w, v, observation_bits<F64>(a, j > last ? j : last, sl.k[v], i));
    }
    return w;
}

template <int V, bool F64>
__global__ __launch_bounds__(kRolloutInputsBlock) void rollout_inputs_dense_kernel(const InputsArgs a) {
    const int64_t chunk = blockIdx.x / a.col_blocks;
    const int64_t c = (blockIdx.x - chunk * a.col_blocks) * kRolloutInputsBlock + threadIdx.x;
    if (c >= a.cols) return;
#if GYMNET_ROLLOUT_INPUTS_LANE_MAJOR
    const int64_t q = c / a.count, i = c - q * a.count;      // the probe's other assignment: neighbouring threads, neighbouring lanes
#else
    const int64_t i = c / a.per_row, q = c - i * a.per_row;
#endif
    const Slots<V> sl(a, q * V);
    const int64_t t0 = chunk * a.rows_per_chunk;
    const int64_t t1 = t0 + a.rows_per_chunk < a.steps ? t0 + a.rows_per_chunk : a.steps;
    int64_t last = last_done_before(a, t0, i);
    // the outputs are no input (the call refuses equal pointers): loads of a later row may pass the stores of an earlier one
    uint32_t *__restrict__ out = a.x + (t0 * a.count + i) * a.x_row_stride + q * V;
    const uint8_t *__restrict__ done = a.rec_done + i;
    const int64_t out_step = a.count * a.x_row_stride;
    for (int64_t t = t0; t < t1; t += kRowsInFlight) {
        uint8_t d[kRowsInFlight];
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) d[u] = t + u < t1 ? done[(t + u) * a.stride] : (uint8_t)0;
        typename Word<V>::T w[kRowsInFlight];
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) {
            if (t + u < t1) {                                  // wave-uniform
                w[u] = input_word<V, F64>(a, sl, t + u, last, i);
                if (d[u] != 0) last = t + u;
            }
        }
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u)
            if (t + u < t1) *reinterpret_cast<typename Word<V>::T *>(out + u * out_step) = w[u];
        out += kRowsInFlight * out_step;
    }
}

template <int V, bool F64>
__global__ __launch_bounds__(kRolloutInputsBlock) void rollout_inputs_gather_kernel(const InputsArgs a) {
    const int64_t c = (int64_t)blockIdx.x * kRolloutInputsBlock + threadIdx.x;
    if (c >= a.cols) return;
    const int64_t j = c / a.per_row, q = c - j * a.per_row;
    const int64_t r = a.rows[j];
    typename Word<V>::T *out = reinterpret_cast<typename Word<V>::T *>(a.x + j * a.x_row_stride + q * V);
    if (r < 0 || r >= a.steps * a.count) {
        typename Word<V>::T nan;
#pragma unroll
        for (int v = 0; v < V; ++v) set_word(nan, v, kCanonicalNaN);
        *out = nan;
        return;
    }
    const int64_t t = r / a.count, i = r - t * a.count;
    const Slots<V> sl(a, q * V);
    *out = input_word<V, F64>(a, sl, t, last_done_before(a, t, i), i);
}

template <bool F64>
__global__ __launch_bounds__(kRolloutInputsBlock) void rollout_inputs_history_kernel(const InputsArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kRolloutInputsBlock + threadIdx.x;
    if (i >= a.count) return;
    const int64_t last = last_done_before(a, a.steps, i);
    uint32_t *__restrict__ out = a.history_out + i;
    for (int32_t s = 0; s < a.history; ++s) {
        const int64_t j = a.steps - a.history + s;
        for (int32_t k = 0; k < a.obs_dim; ++k) out[((int64_t)s * a.obs_dim + k) * a.history_out_stride] = observation_bits<F64>(a, j > last ? j : last, k, i);
    }
}

template <int V, bool F64>
void launch_rows(const RolloutInputsForm &f, const InputsArgs &a, hipStream_t st) {
    const dim3 grid((unsigned)f.blocks), block(kRolloutInputsBlock);
    if (f.gathered) hipLaunchKernelGGL((rollout_inputs_gather_kernel<V, F64>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((rollout_inputs_dense_kernel<V, F64>), grid, block, 0, st, a);
}

hipError_t launch_rollout_inputs(const RolloutInputsForm &f, const InputsArgs &a, hipStream_t st) {
    if (f.rows) {
        if (f.vec == 4) { if (f.f64) launch_rows<4, true>(f, a, st); else launch_rows<4, false>(f, a, st); }
        else            { if (f.f64) launch_rows<1, true>(f, a, st); else launch_rows<1, false>(f, a, st); }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (f.history) {
        const dim3 grid((unsigned)((a.count + kRolloutInputsBlock - 1) / kRolloutInputsBlock)), block(kRolloutInputsBlock);
        if (f.f64) hipLaunchKernelGGL((rollout_inputs_history_kernel<true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((rollout_inputs_history_kernel<false>), grid, block, 0, st, a);
    }
    return hipGetLastError();
}

}  // namespace

}  // namespace gymnet

using namespace gymnet;

extern "C" {

int gymnet_rollout_inputs_device(int device, void *stream, int64_t steps, int64_t count, int64_t stride, int32_t obs_dim, int32_t history,
                                 int32_t obs_f64, const void *d_rec_obs, const uint8_t *d_rec_done, const float *d_history0, int64_t history0_stride,
                                 const int64_t *d_rows, int64_t num_rows, float *d_x, int64_t x_row_stride, float *d_history_out,
                                 int64_t history_out_stride) {
    return guarded([&]() -> int {
    const RolloutInputsCall c{steps, count, stride, obs_dim, history, obs_f64, (uintptr_t)d_rec_obs, (uintptr_t)d_rec_done, (uintptr_t)d_history0,
                              history0_stride, (uintptr_t)d_rows, d_rows ? num_rows : 0, (uintptr_t)d_x, x_row_stride, (uintptr_t)d_history_out,
                              history_out_stride};
    if (const char *why = rollout_inputs_refusal(c)) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "rollout_inputs: %s", why);
    const RolloutInputsForm f = pick_rollout_inputs_form(c, GYMNET_ROLLOUT_INPUTS_TARGET_THREADS);
    if (!f.rows && !f.history) return GYMNET_OK;
    if (f.blocks > 0x7FFFFFFF || (count + kRolloutInputsBlock - 1) / kRolloutInputsBlock > 0x7FFFFFFF)
        return fail(nullptr, GYMNET_ERR_INVALID_ARG, "rollout_inputs: %lld blocks are beyond one launch's grid", (long long)f.blocks);
    const InputsArgs a{d_rec_obs, d_rec_done, reinterpret_cast<const uint32_t *>(d_history0), d_rows, reinterpret_cast<uint32_t *>(d_x),
                       reinterpret_cast<uint32_t *>(d_history_out), steps, count, stride, history0_stride, x_row_stride, history_out_stride,
                       f.cols, f.col_blocks, f.rows_per_chunk, f.per_row, obs_dim, history};
    DeviceScope scope;
    (void)hipGetLastError();
    HIP_TRY(nullptr, hipSetDevice(device));
    HIP_TRY(nullptr, launch_rollout_inputs(f, a, static_cast<hipStream_t>(stream)));
    return GYMNET_OK;
    });
}

}  // extern "C"
