// launch_policy.hpp — the launch configuration a handle starts with, as a pure function of plain values.  Host only: no HIP header, so
// tests/cpp/launch_policy_test.cpp holds every threshold from both sides on a CPU (g++ -std=c++17).  launch_policy.hip gathers the facts
// from a handle and stores the result; kernels.hpp includes this for LaunchCfg.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "../../include/gymnet_amd.h"

namespace gymnet {

// vec: envs per thread (4 = dwordx4 streams, 1 = scalar); block: threads per workgroup;
// nt: non-temporal mask (0 none, 12 action + reward/done streams, 15 every stream)
// lds_bytes: unused dynamic LDS requested per workgroup, for the ONE purpose of capping occupancy in probes (one-shot kernel)
// items: lanes per thread of the fully unrolled software-pipelined kernel (envs with PIPELINED only; 1 = one-shot kernel)
// reset_form: 1 = wave-compacted fused reset in the one-step kernel (reset_pending_wave: envs whose observation aliases the
// state, dwordx4 lanes)
// lds_pipe: 1 = the multi-lane kernel in its producer / consumer form (step_kernel_lds: `items` tiles per workgroup)
// simds: SIMD units of the handle's device (multiProcessorCount x 4; 1024 on MI355X) — sizes the resident generation of the looped
// multi-pair kernel (step_kernels.hpp pipe2_chunks) and the policy's waves-per-SIMD windows (default_policy below)
struct LaunchCfg { int vec; int block; int nt; int lds_bytes = 0; int items = 1; int reset_form = 0; int lds_pipe = 0; int simds = 1024; };

// What default_policy reads of a handle.
struct PolicyFacts {
    int env_id = 0;             // gymnet_env_id: Acrobot is ALU-bound, Pendulum's no-non-temporal window starts later
    bool alias = false;         // the env's observation IS its state (EnvDesc::alias)
    int bytes_per_step = 0;     // algorithmic bytes one env-step moves (handle.hpp bytes_per_step: 73 for a float64 handle)
    bool f64 = false, autoreset = false;
    int64_t n = 0;              // lanes
    int simds = 1024;           // SIMD units of the device
    // float32: every state / observation row (both halves of a double-buffered pair) 16-byte aligned and the strides a multiple of 4;
    // 8-byte aligned and a multiple of 2.  float64: state rows 16-byte aligned and the state stride even.  External buffers may not be.
    bool rows16 = false, rows8 = false, can2_f64 = false;
};
// the configuration, and what the buffers' alignment / the batch size allow a later gymnet_vecenv_set_launch_policy to ask for
struct DefaultPolicy { LaunchCfg cfg{4, 256, 0, 0, 1}; bool can_vec4 = false, can_vec2 = false, lds_ok = false; };

// The launch configuration a handle starts with (gymnet_vecenv_set_launch_policy changes it afterwards).
inline DefaultPolicy default_policy(const PolicyFacts &f) {
    DefaultPolicy out;
    LaunchCfg &lcfg = out.cfg;
    if (f.f64) {
        // float64 CartPole: two lanes per thread (one dwordx4 per state row and direction) where the rows are 16-byte aligned
        // (external observation buffers may not be); stream policy by the bytes a vector step moves, with the thresholds of the
        // float32 path below
        const size_t step_bytes = (size_t)f.n * (size_t)f.bytes_per_step;
        const bool can2 = f.can2_f64;
        out.can_vec4 = false; out.can_vec2 = can2; out.lds_ok = false;
        // measured at 2^20 lanes (73 MiB per step; us per step, gpurun_out r4): every stream non-temporal 14.3, state cacheable 14.8,
        // nothing non-temporal 16.2, one lane per thread 15.6
        // reset_form 1 (two lanes per reset in the wave-compacted form, step_kernels.hpp) for the one-shot kernel and the fused rollout:
        // one-shot 13.7 -> 13.4 us at 2^20 lanes, bookkeeping rollout 7.5 -> 6.9 us per step, lean rollout 5.9 -> 6.0
        // (profiles/rollout_reset_forms_r05.txt); the multi-pair kernel below always draws once per thread-group of pairs
        lcfg = LaunchCfg{can2 ? 2 : 1, 256, 15, 0, 1, can2 ? 1 : 0, 0, f.simds};
        // Stream policy by the bytes a vector step moves (round 6, profiles/f64_sizes_r06.txt; us per 2^20 lanes, one-shot kernel,
        // nothing non-temporal | state cacheable (12) | every stream non-temporal (15)):
        //   2^21 lanes 12.9 | 14.8 | 13.7     3 * 2^20  11.8 | 13.4 | 12.6     2^22  12.1 | 13.8 | 14.1     2^23  13.1 | 13.5 | 12.6
        // While everything a step touches fits the 256 MiB Infinity Cache (<= 300 MiB moved: the state is rewritten in place), plain
        // cacheable accesses win by 6-13 % — the next launch finds its inputs on the die; beyond it nothing can stay and every stream
        // is marked non-temporal (rounds 4-5 kept the state cacheable between 96 and 768 MiB: 4-7 % slower at every size measured).
        if (step_bytes > ((size_t)96 << 20) && step_bytes <= ((size_t)300 << 20)) lcfg.nt = 0;
        // The multi-pair kernel (step_kernel_pipe2<CartPole64, k>: a thread owns k lane pairs, all loads first, then advance pair after
        // pair, ONE wave-compacted reset for all of them, then the state rows) wins where it runs as ONE resident generation that fills
        // the chip: four pairs hold 185 VGPRs = two waves per SIMD (2048 waves of 512 lanes), two pairs three (3072 waves of 256 lanes).
        // us per step, one-shot | 2 pairs | 4 pairs (profiles/f64_sizes_r05.txt, one box):
        //   2^19 lanes 6.27 | 6.42 | 7.57      3 * 2^18  10.94 | 8.46 | 10.19      2^20  13.13 | 12.17 | 11.19
        //   5 * 2^18   16.64 | 16.82 | 17.40   6 * 2^18  21.17 | 19.78 | 19.58     2^21  27.72 | 28.56 | 29.64   (larger: one-shot)
        // (round 4, 271 VALU per env-step, per-pair drain-loop reset: one-shot 14.4, 2 pairs 13.1, 4 pairs 14.4 at 2^20; round 5 before
        // the deferred reset: 13.4-13.6 | 13.1-13.4 | 12.8-13.2.)  Lean variant only; without auto-reset whole 2 * k * 256-lane groups
        // only (the launcher falls back otherwise).  A wave count just under a whole number per SIMD is as good (10^6 lanes: 11.7 us against 13.0).
        // Beyond one generation the kernel is launched slice by slice (step_kernels.hpp pipe2_chunks) and is no faster than the one-shot
        // kernel — 2^21 lanes: 27.9 us in two slices, 35.2 as a looping grid, 27.4 one-shot with the same mask, 25.8 one-shot
        // cacheable (profiles/f64_sizes_r06.txt): what makes 2^20 lanes fast is that the launch's written lines fit the L2s and leave
        // after the kernel, not the launch shape — so it is not selected there.  (Round 5's window test also let FOUR pairs through at
        // three waves per SIMD, which they cannot hold: 3 * 2^19 lanes ran at 16.6 us per 2^20 lanes against 13.3.  Fixed.)
        if (can2 && f.n >= ((int64_t)3 << 18)) {            // (below: ramp-bound, fewer and fatter waves lose)
            for (int items : {4, 2}) {
                if (!f.autoreset && f.n % ((int64_t)512 * items) != 0) continue;     // (the auto-reset form takes any batch size)
                const double waves_per_simd = (double)((f.n + 128 * items - 1) / ((int64_t)128 * items)) / (double)f.simds;   // MI355X: 256 CUs x 4 SIMDs
                // NOT one wave more: the kernel holds 191 VGPRs, two waves per SIMD are resident, and a 2049th wave starts when an
                // earlier one has finished — 2^20 + 2 lanes: 19.2 us against 11.1 (profiles/f64_sizes_r05.txt, second table)
                const bool fills = items == 4 ? (waves_per_simd >= 1.9 && waves_per_simd <= 2.0) : (waves_per_simd >= 2.85 && waves_per_simd <= 3.0);
                if (fills) { lcfg.items = items; lcfg.nt = 15; break; }
            }
        }
        return out;
    }
    // dwordx4 streams need 16-byte aligned component arrays; external buffers may not be
    const bool can_vec4 = f.rows16;
    // Launch policy, measured on MI355X with tools/probe_step.hip and bench.py (profiles/probe_r01.txt),
    // keyed on the bytes one vector step moves (lanes x algorithmic bytes per env-step):
    //  - <= 2^19 lanes (round 1-4: "<= 24 MiB per vector step"): scalar lanes — 4x the waves hide latency better than dwordx4 on a small grid;
    //  - <= 48 MiB (2^20 CartPole lanes): dwordx4, every stream non-temporal;
    //  - <= 300 MiB (the step's whole footprint fits the 256 MiB Infinity Cache): dwordx4, nothing non-temporal (round 6);
    //  - <= 768 MiB (the state fits it): dwordx4, state cacheable, action / reward / done streamed
    //    past it, so the next launch re-reads the state from the cache;
    //  - larger: nothing can stay resident — scalar lanes, every stream non-temporal;
    //  - Acrobot (RK4, ALU-bound: ~650 VALU per env-step) always takes scalar lanes: 21.7 vs 27.7 us at 2^20.
    const size_t step_bytes = (size_t)f.n * (size_t)f.bytes_per_step;
    const bool alu_bound = f.env_id == GYMNET_ENV_ACROBOT;
    lcfg.simds = f.simds;
    // Round 5: the small-batch rule is a LANE count, not a byte count.  Scalar lanes win while the launch is ONE resident generation
    // of waves — n <= 8 waves x 1024 SIMDs x 64 lanes = 2^19 — and lose beyond it (a second generation of 64-lane waves starts when the
    // first retires); the byte threshold had been fitted on CartPole alone (2^19 lanes = 21.5 MB) and kept MountainCar (25 B per lane)
    // on scalar lanes up to 10^6 lanes: 5.53 us against 4.53 with 16-byte lanes; 3 * 2^18 lanes 4.35 against 3.93
    // (profiles/small_batches_r05.txt; CartPole and Pendulum cross over at the same lane count).
    const bool one_generation = f.n <= ((int64_t)8 * f.simds * 64);
    if (alu_bound || one_generation) { lcfg.vec = 1; lcfg.nt = 15; }
    // Round 6 (profiles/trough_r06.txt): while everything a step touches fits the 256 MiB Infinity Cache — up to ~300 MiB
    // moved, the state being rewritten in place — and the launch is more than ~1.25 generations of waves, NO stream is marked
    // non-temporal.  us per 2^20 lanes, mask 0 against the former choice (15 up to 48 MiB, 12 beyond), two boxes:
    //   CartPole     5 * 2^18 lanes 6.26 / 6.56   2^21 7.03 / 7.33   3 * 2^20 6.86 / 7.54   2^22 6.72 / 7.24   6 * 2^20 6.40 / 6.78
    //                2^23 6.80 / 6.85 (the crossover)   2^24 7.96 / 6.52 (mask 12 stays)
    //   MountainCar  3 * 2^19 4.31 / 5.10   2^21 3.83 / 4.48   2^22 4.14 / 4.33   2^23 3.92 / 4.10   2^24 3.85 / 3.87
    //   Pendulum     3 * 2^19 5.93 / 5.42 and 2^21 6.05 / 5.30 (loses: two of its four written rows are never read back),
    //                2^22 5.51 / 6.27   2^23 5.68 / 5.68 — hence its later start
    // MountainCarContinuous moves MountainCar's 25 B per env-step and takes MountainCar's rule throughout.  Measured beside it in one run
    // (profiles/mountaincar_continuous.txt, us per step, MountainCar / MountainCarContinuous): 2^19 lanes 4.51 / 4.50, 5 * 2^18 5.84 / 5.93,
    // 2^20 4.79 / 4.67, 2^22 18.16 / 18.09 — the same kernels of both envs land within 2 % of each other at every size.
    else if (f.n >= (f.env_id == GYMNET_ENV_PENDULUM ? (int64_t)3 << 20 : (int64_t)5 << 18) && step_bytes <= ((size_t)300 << 20)) { lcfg.vec = 4; lcfg.nt = 0; }
    else if (step_bytes <= ((size_t)48 << 20)) { lcfg.vec = 4; lcfg.nt = 15; }
    else if (step_bytes <= ((size_t)768 << 20)) { lcfg.vec = 4; lcfg.nt = 12; }
    else { lcfg.vec = 1; lcfg.nt = 15; }
    if (!can_vec4) lcfg.vec = 1;
    // Acrobot's wide form is TWO lanes per thread whose arithmetic rides the packed FP32 instructions (envs.hpp).  Opt-in
    // (gymnet_launch_policy.vec = 2): bit-identical, 287 instead of 454 VALU per env-step, and slower — 15.0 vs 14.2 us at 2^20
    // lanes, 13.6 vs 12.3 us per 2^20 lanes at 2^23 (profiles/acrobot_probes_r02.txt, docs/ledger.md §4a).
    const bool can_vec2 = f.rows8;
    // Acrobot's multi-lane kernel (step_kernel_pipe: all loads first, then compute / store lane after lane) wins where the
    // one-shot kernel would run as ~2 lock-step wave generations: it turns the launch into ONE generation of 4096 waves whose
    // stores drain under the next lane's arithmetic.  Measured (profiles/acrobot_probes_r02.txt, us per 2^20 lanes, one-shot
    // vs k = ceil(n / 2^18) lanes per thread): n = 2^19 15.1 vs 14.5, 3*2^18 13.9 vs 13.9, 2^20 14.9 vs 13.1, 5*2^18 13.7 vs
    // 13.1; beyond that the one-shot kernel's generations overlap by themselves (6*2^18: 13.7 vs 13.8; 2^21: 13.4 vs 13.3).
    // k is n / 2^18 ROUNDED, not rounded up: one lane more than 2^20 used to select k = 5 — 17.5 us per step against 12.5 at 2^20 lanes
    // (profiles/ragged_r05.txt); with k = 4 the 4097th workgroup is one more wave on a chip that holds eight per SIMD.
    if (alu_bound && f.n >= ((int64_t)1 << 19) && f.n < ((int64_t)11 << 17)) lcfg.items = (int)((f.n + ((int64_t)1 << 17)) >> 18);
    // Wave-compacted fused reset (kernels.hip: reset_pending_wave) wherever the dwordx4 lean kernel of an env whose observation IS
    // its state runs: the wave's finished sub-lanes are drawn in ONE Philox pass by its first lanes instead of 1.6 mostly idle
    // passes.  CartPole at 2^20 lanes: 6.91 -> 6.52 us per launch, bit-identical (profiles/forms_probe_r03.txt).
    lcfg.reset_form = (f.alias && lcfg.vec == 4) ? 1 : 0;
    // producer / consumer form of the multi-lane kernel (opt-in, gymnet_launch_policy.lds_pipe = 1): whole 512-lane tiles and
    // 16-byte aligned rows only.  Bit-identical and SLOWER at 2^20 lanes — 13.5-14.9 vs 11.7-12.7 us (profiles/acrobot_lds_r03.txt):
    // the computing waves' waits on memory instructions drop from 34 % to 21 % of their cycles, the s_barrier per tile adds more.
    const bool lds_ok = alu_bound && can_vec4 && (f.n % 512) == 0;
    // 64-thread workgroups for the dwordx4 kernels of the smallest payloads (< 40 MiB per vector step at dwordx4: MountainCar and
    // Pendulum at 2^20 lanes): such a launch is ramp / drain bound, and one-wave workgroups ramp and retire faster — MountainCar 4.92-5.05
    // -> 4.55-4.73 us, Pendulum 5.97 -> 5.88 us; CartPole (41 MiB) does not gain (tools/gpu_nt_ab_r03.sh, profiles/block_nt_probe_r03.txt)
    if (lcfg.vec == 4 && step_bytes < ((size_t)40 << 20)) lcfg.block = 64;
    out.can_vec4 = can_vec4; out.can_vec2 = can_vec2; out.lds_ok = lds_ok;
    return out;
}

}  // namespace gymnet
