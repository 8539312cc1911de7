// rollout_inputs.hpp — what a call to gymnet_rollout_inputs_device is refused for, and which form of the kernels of rollout_inputs.hip it
// launches.  Host-only and pure: no HIP type, no global, nothing read but the arguments, so tests/cpp/rollout_inputs_test.cpp runs it as a
// stand-alone program.  This is the only place that refuses a call or picks its form.
//
// An output row is width = history * obs_dim floats.  One thread owns V consecutive floats of it — of one lane's row in the dense form,
// walking a chunk of rows t; of one gathered row in the gathered form — and consecutive threads own consecutive floats, so that where
// x_row_stride == width a wave's store instruction covers 64 * V * 4 contiguous bytes.  V = 4 (16-byte stores) needs every thread's four
// floats to start a 16-byte unit of d_x, which holds exactly when
//     width % 4 == 0,  x_row_stride % 4 == 0,  d_x is 16-byte aligned.
// Anything else runs V = 1.  The inputs are read 4 (float64: 8) bytes at a time in either form: their alignment beyond what the call
// demands decides nothing.  The dense form cuts the steps into chunks of rows_per_chunk so that a small batch still fills the device; a
// chunk is never shorter than the history (the look-back at its start reads at most history - 1 done bytes) or than kRolloutInputsMinRows.
#pragma once
#include <cstdint>

namespace gymnet {

struct RolloutInputsCall {                        // the call's arguments; pointers as integers, 0 = NULL
    int64_t steps, count, stride;
    int32_t obs_dim, history, obs_f64;
    uintptr_t rec_obs, rec_done, history0;
    int64_t history0_stride;
    uintptr_t rows;
    int64_t num_rows;
    uintptr_t x;
    int64_t x_row_stride;
    uintptr_t history_out;
    int64_t history_out_stride;
};

struct RolloutInputsForm {
    int vec;                                      // floats of an output row per thread: 1 or 4
    bool f64, gathered;
    bool rows, history;                           // which kernels run: the dense / gathered one, the one that writes d_history_out
    int64_t per_row;                              // threads per output row: width / vec
    int64_t cols;                                 // dense: count * per_row, gathered: num_rows * per_row
    int64_t col_blocks;                           // cols in blocks of 256 threads
    int64_t rows_per_chunk, chunks;               // dense: rows t a thread walks, and how many such chunks cover the steps; gathered: 1, 1
    int64_t blocks;                               // col_blocks * chunks
};

constexpr int kRolloutInputsBlock = 256;
constexpr int kRolloutInputsMaxWidth = 64;        // the widest input an actor can have (actor_net.hpp kActorMaxWidth)
constexpr int64_t kRolloutInputsMinRows = 8;
// threads the dense form asks for before it lets a thread walk more rows: 32 waves of 64 for each of an MI355X's 1024 SIMDs, four times
// what is resident at once.  Measured (docs/ledger.md §rollout inputs): at 2^16 lanes x 256 steps eight chunks of 32 rows take 429 us, two of
// 128 rows 464, one of 256 rows 433; at 2^20 lanes the lanes alone exceed either target.
constexpr int64_t kRolloutInputsTargetThreads = 32 * 64 * 1024;

// NULL: the call is accepted; else why it is refused (GYMNET_ERR_INVALID_ARG, "rollout_inputs: <this>").  Nothing is written by a refused call.
inline const char *rollout_inputs_refusal(const RolloutInputsCall &c) {
    const bool gathered = c.rows != 0;
    if (c.steps < 0 || c.count < 0 || c.stride < 0 || c.history0_stride < 0 || c.x_row_stride < 0 || c.history_out_stride < 0 || c.num_rows < 0)
        return "a size or stride is negative";
    if (c.obs_dim < 1 || c.history < 1) return "obs_dim and history must be >= 1";
    if ((int64_t)c.obs_dim * c.history > kRolloutInputsMaxWidth) return "history * obs_dim is beyond 64, the widest input an actor can have";
    const int64_t width = (int64_t)c.obs_dim * c.history;
    if (c.stride < c.count) return "stride < count";
    if (c.history0 && c.history0_stride < c.count) return "history0_stride < count";
    if (c.history_out && c.history_out_stride < c.count) return "history_out_stride < count";
    const bool any = c.steps > 0 && c.count > 0;                              // there are recorded rows
    const bool writes_rows = any && (!gathered || c.num_rows > 0);
    if (c.steps > 0 && (!c.rec_obs || !c.rec_done || !c.history0)) return "d_rec_obs / d_rec_done / d_history0 is null with steps > 0";
    if (c.history_out && !c.history0) return "d_history_out needs d_history0";
    if (writes_rows && !c.x) return "d_x is null where rows are to be written";
    if (writes_rows && c.x_row_stride < width) return "x_row_stride < history * obs_dim";
    if ((c.rec_obs & (c.obs_f64 ? 7u : 3u)) != 0) return c.obs_f64 ? "d_rec_obs must be 8-byte aligned (float64 observations)" : "d_rec_obs must be 4-byte aligned";
    if (((c.history0 | c.x | c.history_out) & 3u) != 0) return "d_history0, d_x and d_history_out must be 4-byte aligned";
    if ((c.rows & 7u) != 0) return "d_rows must be 8-byte aligned";
    for (const uintptr_t out : {c.x, c.history_out}) {
        if (!out) continue;
        if (out == c.rec_obs || out == c.rec_done || out == c.history0 || out == c.rows) return "an output may not alias an input";
    }
    if (c.x && c.x == c.history_out) return "d_x and d_history_out are the same array";
    // every element offset the kernels form fits an int64: [steps][obs_dim][stride] 8-byte observations, rows of x_row_stride floats
    if (any && c.stride > 0 && c.steps > INT64_MAX / 8 / c.obs_dim / c.stride) return "steps x obs_dim x stride overflows";
    if (writes_rows && c.x_row_stride > 0) {
        const int64_t out_rows = gathered ? c.num_rows : c.steps * c.count;   // (steps * count <= steps * stride: checked above)
        if (out_rows > INT64_MAX / 4 / c.x_row_stride) return "the output rows x x_row_stride overflow";
    }
    return nullptr;
}

// the form of an accepted call
inline RolloutInputsForm pick_rollout_inputs_form(const RolloutInputsCall &c, int64_t target_threads = kRolloutInputsTargetThreads) {
    RolloutInputsForm f{};
    const int64_t width = (int64_t)c.obs_dim * c.history;
    const bool any = c.steps > 0 && c.count > 0;
    f.gathered = c.rows != 0;
    f.f64 = c.obs_f64 != 0;
    f.rows = any && (!f.gathered || c.num_rows > 0);
    f.history = c.history_out != 0 && c.count > 0 && !(f.gathered && c.num_rows == 0);
    f.vec = width % 4 == 0 && c.x_row_stride % 4 == 0 && (c.x & 15u) == 0 ? 4 : 1;
    f.per_row = width / f.vec;
    f.rows_per_chunk = f.chunks = 1;
    if (!f.rows) return f;                                                    // cols = blocks = 0: no row kernel
    f.cols = (f.gathered ? c.num_rows : c.count) * f.per_row;
    f.col_blocks = (f.cols + kRolloutInputsBlock - 1) / kRolloutInputsBlock;
    if (!f.gathered) {
        const int64_t per_chunk = f.col_blocks * kRolloutInputsBlock;
        const int64_t want = target_threads > per_chunk ? (target_threads + per_chunk - 1) / per_chunk : 1;   // chunks that reach the target
        int64_t r = (c.steps + want - 1) / want;
        const int64_t floor_rows = c.history > kRolloutInputsMinRows ? c.history : kRolloutInputsMinRows;
        if (r < floor_rows) r = floor_rows;
        if (r > c.steps) r = c.steps;
        f.rows_per_chunk = r;
        f.chunks = (c.steps + r - 1) / r;
    }
    f.blocks = f.col_blocks * f.chunks;
    return f;
}

}  // namespace gymnet
