// rollout_inputs_test.cpp — the host side of gymnet_rollout_inputs_device that needs no library: the refusals (rollout_inputs_refusal)
// and the form picker (pick_rollout_inputs_form) of gym.net_amd/csrc/rollout_inputs.hpp, host-only and pure.  Stand-alone: g++ -std=c++17,
// nothing linked.  Every rule of the picker from both sides, and every refusal with its text.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "rollout_inputs.hpp"

using gymnet::RolloutInputsCall;
using gymnet::RolloutInputsForm;

static int failed = 0;
#define CHECK(cond, msg)                                                          \
    do {                                                                          \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, msg); ++failed; } \
    } while (0)

// an accepted dense call: CartPole at S = 4, 1028 lanes, 37 steps
static RolloutInputsCall good() {
    RolloutInputsCall c{};
    c.steps = 37; c.count = 1028; c.stride = 1028;
    c.obs_dim = 4; c.history = 4; c.obs_f64 = 0;
    c.rec_obs = 0x10000; c.rec_done = 0x20000; c.history0 = 0x30000; c.history0_stride = 1028;
    c.rows = 0; c.num_rows = 0;
    c.x = 0x40000; c.x_row_stride = 16;
    c.history_out = 0x50000; c.history_out_stride = 1028;
    return c;
}

static bool refused(const RolloutInputsCall &c, const char *word) {
    const char *why = gymnet::rollout_inputs_refusal(c);
    return why && std::strstr(why, word);
}

static void refusal_checks() {
    CHECK(gymnet::rollout_inputs_refusal(good()) == nullptr, "the good call is accepted");
    RolloutInputsCall c;
    int64_t RolloutInputsCall::*sizes[] = {&RolloutInputsCall::steps, &RolloutInputsCall::count, &RolloutInputsCall::stride, &RolloutInputsCall::history0_stride,
                                           &RolloutInputsCall::x_row_stride, &RolloutInputsCall::history_out_stride};
    for (auto m : sizes) { c = good(); c.*m = -1; CHECK(refused(c, "negative"), "a negative size"); }
    c = good(); c.rows = 0x60000; c.num_rows = -1; CHECK(refused(c, "negative"), "negative num_rows");
    c = good(); c.obs_dim = 0; CHECK(refused(c, "must be >= 1"), "obs_dim 0");
    c = good(); c.history = 0; CHECK(refused(c, "must be >= 1"), "history 0");
    c = good(); c.history = -3; CHECK(refused(c, "must be >= 1"), "history < 0");
    c = good(); c.history = 17; c.x_row_stride = 68; CHECK(refused(c, "beyond 64"), "4 x 17 = 68 floats");
    c = good(); c.history = 16; c.x_row_stride = 64; CHECK(!gymnet::rollout_inputs_refusal(c), "4 x 16 = 64 floats is the widest input");
    c = good(); c.obs_dim = 1; c.history = 64; c.x_row_stride = 64; CHECK(!gymnet::rollout_inputs_refusal(c), "1 x 64 too");
    c = good(); c.obs_dim = 1 << 30; c.history = 1 << 30; CHECK(refused(c, "beyond 64"), "a product that leaves int32");
    c = good(); c.stride = 1027; CHECK(refused(c, "stride < count"), "stride < count");
    c = good(); c.history0_stride = 1027; CHECK(refused(c, "history0_stride < count"), "history0_stride < count");
    c = good(); c.history_out_stride = 1027; CHECK(refused(c, "history_out_stride < count"), "history_out_stride < count");
    c = good(); c.history_out = 0; c.history_out_stride = 0; CHECK(!gymnet::rollout_inputs_refusal(c), "... which is not looked at without d_history_out");
    c = good(); c.x_row_stride = 15; CHECK(refused(c, "x_row_stride <"), "x_row_stride below the row width");
    c = good(); c.x_row_stride = 19; CHECK(!gymnet::rollout_inputs_refusal(c), "... and above it");
    c = good(); c.rec_obs = 0; CHECK(refused(c, "null with steps > 0"), "null d_rec_obs");
    c = good(); c.rec_done = 0; CHECK(refused(c, "null with steps > 0"), "null d_rec_done");
    c = good(); c.history0 = 0; CHECK(refused(c, "null with steps > 0"), "null d_history0");
    c = good(); c.steps = 0; c.rec_obs = c.rec_done = 0; CHECK(!gymnet::rollout_inputs_refusal(c), "steps == 0 needs neither record");
    c = good(); c.steps = 0; c.history0 = 0; CHECK(refused(c, "needs d_history0"), "steps == 0 with d_history_out still needs d_history0");
    c = good(); c.steps = 0; c.history0 = 0; c.history_out = 0; CHECK(!gymnet::rollout_inputs_refusal(c), "steps == 0, nothing asked for");
    c = good(); c.x = 0; CHECK(refused(c, "d_x is null"), "null d_x, dense");
    c = good(); c.x = 0; c.rows = 0x60000; c.num_rows = 5; CHECK(refused(c, "d_x is null"), "null d_x, gathered");
    c = good(); c.x = 0; c.rows = 0x60000; c.num_rows = 0; CHECK(!gymnet::rollout_inputs_refusal(c), "the gathered form with no rows writes no row");
    c = good(); c.x = 0; c.x_row_stride = 0; c.steps = 0; CHECK(!gymnet::rollout_inputs_refusal(c), "steps == 0: d_x and its stride are not looked at");
    c = good(); c.x = 0; c.x_row_stride = 0; c.count = 0; c.stride = 0; CHECK(!gymnet::rollout_inputs_refusal(c), "count == 0 likewise");
    for (uintptr_t off : {1, 2, 3}) {
        c = good(); c.rec_obs += off; CHECK(refused(c, "d_rec_obs must be 4-byte"), "float32 d_rec_obs off 4 bytes");
        c = good(); c.history0 += off; CHECK(refused(c, "4-byte aligned"), "d_history0 off 4 bytes");
        c = good(); c.x += off; CHECK(refused(c, "4-byte aligned"), "d_x off 4 bytes");
        c = good(); c.history_out += off; CHECK(refused(c, "4-byte aligned"), "d_history_out off 4 bytes");
        c = good(); c.rec_done += off; CHECK(!gymnet::rollout_inputs_refusal(c), "d_rec_done may start at any byte");
    }
    for (uintptr_t off : {1, 2, 4, 7}) {
        c = good(); c.obs_f64 = 1; c.rec_obs += off; CHECK(refused(c, "8-byte aligned (float64"), "float64 d_rec_obs off 8 bytes");
        c = good(); c.rows = 0x60000 + off; c.num_rows = 3; CHECK(refused(c, "d_rows must be 8-byte"), "d_rows off 8 bytes");
    }
    c = good(); c.rec_obs += 4; CHECK(!gymnet::rollout_inputs_refusal(c), "float32 d_rec_obs needs 4 bytes only");
    c = good(); c.obs_f64 = 1; c.rec_obs += 8; CHECK(!gymnet::rollout_inputs_refusal(c), "float64 d_rec_obs on the next 8-byte boundary");
    uintptr_t RolloutInputsCall::*outs[] = {&RolloutInputsCall::x, &RolloutInputsCall::history_out};
    uintptr_t RolloutInputsCall::*ins[] = {&RolloutInputsCall::rec_obs, &RolloutInputsCall::rec_done, &RolloutInputsCall::history0, &RolloutInputsCall::rows};
    for (auto o : outs)
        for (auto i : ins) {
            c = good(); c.rows = 0x60000; c.num_rows = 3; c.*o = c.*i;
            CHECK(refused(c, "alias"), "an output equal to an input");
        }
    c = good(); c.history_out = c.x; CHECK(refused(c, "same array"), "d_x == d_history_out");
    c = good(); c.steps = INT64_MAX / 4; c.stride = c.count = 4; c.history0_stride = c.history_out_stride = 4; CHECK(refused(c, "overflows"), "steps x obs_dim x stride beyond int64");
    c = good(); c.x_row_stride = INT64_MAX / 1000; CHECK(refused(c, "overflow"), "rows x x_row_stride beyond int64");
    c = good(); c.rows = 0x60000; c.num_rows = INT64_MAX / 16; CHECK(refused(c, "overflow"), "num_rows x x_row_stride beyond int64");
}

static void picker_checks() {
    RolloutInputsCall c = good();
    RolloutInputsForm f = gymnet::pick_rollout_inputs_form(c);
    CHECK(f.vec == 4 && !f.f64 && !f.gathered && f.rows && f.history, "aligned, divisible: four floats per thread, both kernels");
    CHECK(f.per_row == 4 && f.cols == 1028 * 4 && f.col_blocks == 17, "four threads per row; 4112 threads are 16 blocks and one of 16 threads");
    // 17 blocks of 256 = 4352 threads per chunk; 2097152 / 4352 rounds up to 482 chunks wanted: 1 row each, lifted to the floor of 8
    CHECK(f.rows_per_chunk == 8 && f.chunks == 5 && f.blocks == 85, "37 steps in chunks of 8 rows");
    // the three rules of vec = 4, one at a time, from both sides
    for (int64_t pad : {1, 2, 3, 5}) { c = good(); c.x_row_stride = 16 + pad; CHECK(gymnet::pick_rollout_inputs_form(c).vec == 1, "x_row_stride % 4 != 0: one float per thread"); }
    for (int64_t pad : {4, 8}) { c = good(); c.x_row_stride = 16 + pad; CHECK(gymnet::pick_rollout_inputs_form(c).vec == 4, "x_row_stride % 4 == 0 survives"); }
    for (uintptr_t off : {4, 8, 12}) { c = good(); c.x += off; CHECK(gymnet::pick_rollout_inputs_form(c).vec == 1, "d_x off its 16-byte boundary"); }
    c = good(); c.x += 16; CHECK(gymnet::pick_rollout_inputs_form(c).vec == 4, "... and on the next one");
    c = good(); c.obs_dim = 3; c.history = 21; c.x_row_stride = 64; f = gymnet::pick_rollout_inputs_form(c);
    CHECK(f.vec == 1 && f.per_row == 63 && f.cols == 1028 * 63, "a width of 63: one float per thread");
    c = good(); c.obs_dim = 6; c.history = 4; c.x_row_stride = 24; f = gymnet::pick_rollout_inputs_form(c);
    CHECK(f.vec == 4 && f.per_row == 6, "a width of 24: four, though obs_dim % 4 != 0");
    c = good(); c.obs_dim = 6; c.history = 3; c.x_row_stride = 20; CHECK(gymnet::pick_rollout_inputs_form(c).vec == 1, "a width of 18");
    // what decides nothing: the inputs' alignment, the strides of the inputs, the lane count
    c = good(); c.rec_obs += 4; c.history0 += 4; c.rec_done += 1; c.stride = 1033; c.history0_stride = 1031; c.history_out += 4; c.history_out_stride = 1029;
    CHECK(gymnet::pick_rollout_inputs_form(c).vec == 4, "the inputs' alignment and strides decide nothing");
    for (int64_t n : {(int64_t)1, (int64_t)3, (int64_t)67, (int64_t)1 << 20}) {
        c = good(); c.count = c.stride = c.history0_stride = c.history_out_stride = n; f = gymnet::pick_rollout_inputs_form(c);
        CHECK(f.vec == 4 && f.cols == 4 * n && f.col_blocks == (4 * n + 255) / 256, "any lane count: four floats per thread");
    }
    // float64 and gathered are read off the call
    c = good(); c.obs_f64 = 1; CHECK(gymnet::pick_rollout_inputs_form(c).f64, "obs_f64");
    c = good(); c.obs_f64 = -5; CHECK(gymnet::pick_rollout_inputs_form(c).f64, "any non-zero obs_f64");
    c = good(); c.rows = 0x60000; c.num_rows = 1000; f = gymnet::pick_rollout_inputs_form(c);
    CHECK(f.gathered && f.rows && f.history && f.cols == 4000 && f.col_blocks == 16 && f.chunks == 1 && f.rows_per_chunk == 1 && f.blocks == 16, "gathered: one thread per four floats of a row");
    c.num_rows = 1; f = gymnet::pick_rollout_inputs_form(c); CHECK(f.cols == 4 && f.blocks == 1, "one gathered row");
    c.num_rows = 0; f = gymnet::pick_rollout_inputs_form(c); CHECK(!f.rows && !f.history && f.blocks == 0, "gathered with no row: a no-op, d_history_out included");
    // what runs when there are no recorded rows
    c = good(); c.steps = 0; f = gymnet::pick_rollout_inputs_form(c); CHECK(!f.rows && f.history && f.blocks == 0, "steps == 0: d_history_out only");
    c = good(); c.steps = 0; c.rows = 0x60000; c.num_rows = 7; f = gymnet::pick_rollout_inputs_form(c); CHECK(!f.rows && f.history, "... in the gathered form too");
    c = good(); c.count = 0; f = gymnet::pick_rollout_inputs_form(c); CHECK(!f.rows && !f.history, "count == 0: nothing");
    c = good(); c.history_out = 0; f = gymnet::pick_rollout_inputs_form(c); CHECK(f.rows && !f.history, "no d_history_out: the row kernel alone");
    // the chunks of the dense form: never shorter than the history or kRolloutInputsMinRows, never longer than the steps, and as few
    // rows as reach the target
    CHECK(gymnet::kRolloutInputsMinRows == 8 && gymnet::kRolloutInputsTargetThreads == 32 * 64 * 1024, "the constants");
    c = good(); c.steps = 5; f = gymnet::pick_rollout_inputs_form(c); CHECK(f.rows_per_chunk == 5 && f.chunks == 1, "fewer steps than the floor: one chunk");
    c = good(); c.steps = 8; f = gymnet::pick_rollout_inputs_form(c); CHECK(f.rows_per_chunk == 8 && f.chunks == 1, "exactly the floor");
    c = good(); c.steps = 9; f = gymnet::pick_rollout_inputs_form(c); CHECK(f.rows_per_chunk == 8 && f.chunks == 2, "one row more: a second chunk of one row");
    c = good(); c.obs_dim = 2; c.history = 32; c.x_row_stride = 64; c.steps = 100; f = gymnet::pick_rollout_inputs_form(c);
    CHECK(f.rows_per_chunk == 32 && f.chunks == 4, "a history above the floor is the floor");
    c = good(); c.count = c.stride = c.history0_stride = c.history_out_stride = (int64_t)1 << 20; c.steps = 16; f = gymnet::pick_rollout_inputs_form(c);
    CHECK(f.rows_per_chunk == 16 && f.chunks == 1 && f.blocks == 16384, "2^20 lanes reach the target alone: one chunk");
    c.count = c.stride = c.history0_stride = c.history_out_stride = (int64_t)1 << 16; c.steps = 256; f = gymnet::pick_rollout_inputs_form(c);
    CHECK(f.col_blocks == 1024 && f.rows_per_chunk == 32 && f.chunks == 8 && f.blocks == 8192, "2^16 lanes x 256 steps: eight chunks of 32 rows");
    f = gymnet::pick_rollout_inputs_form(c, 8 * 64 * 1024); CHECK(f.rows_per_chunk == 128 && f.chunks == 2, "a quarter of the target: two chunks of 128 rows");
    f = gymnet::pick_rollout_inputs_form(c, 0); CHECK(f.rows_per_chunk == 256 && f.chunks == 1, "a target of 0: one chunk");
    f = gymnet::pick_rollout_inputs_form(c, (int64_t)1 << 40); CHECK(f.rows_per_chunk == 8 && f.chunks == 32, "a huge target: the floor");
}

int main() {
    refusal_checks();
    picker_checks();
    std::printf("rollout_inputs: %d failed\n", failed);
    return failed ? 1 : 0;
}
