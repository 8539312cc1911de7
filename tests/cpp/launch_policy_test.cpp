// launch_policy_test.cpp — the default launch policy (gym.net_amd/csrc/launch_policy.hpp), a pure function, held to a table on the CPU:
// every threshold from both sides.  g++ -std=c++17, no library, no HIP.
//
// Expected values were produced ONCE by the function as it stood in capi.hip before it became this header (its text behind a shim handle
// in a scratch harness, which also compared both over 786940 argument tuples: docs/ledger.md §32) — never by the code under test.  A rule
// that moves on purpose changes its rows here, with the measurement that moves it.
//
// Rows named "gpu ..." are the 22 of tests/test_gpu_f64_modes.py::test_default_launch_policy_by_batch_size; the kernel name that test
// expects encodes the same fields: step_kernel<Env,VEC,..,NT,RESETF>, step_kernel_pipe<Env,ITEMS,..,NT>, step_kernel_pipe2<Env,ITEMS,..,NT>.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../gym.net_amd/csrc/launch_policy.hpp"

using namespace gymnet;

namespace {

// what capi.hip's kEnvs says of each env: the observation aliases the state, algorithmic bytes per env-step (float64 CartPole: 73)
struct EnvFacts { bool alias; int bytes; };
const EnvFacts kEnvFacts[5] = {{true, 41}, {false, 37}, {true, 25}, {false, 65}, {true, 25}};

// align: 0 = every row on a 16-byte line, even strides; 1 = rows 8 bytes off a line; 2 = rows 4 bytes off (float32 only)
struct Row {
    const char *name;
    int env; bool f64, autoreset; int align, simds; int64_t n;
    int vec, block, nt, items, reset_form; bool lds_ok;
};

const Row kRows[] = {
    {"gpu MountainCar 2^19", GYMNET_ENV_MOUNTAINCAR, false, true, 0, 1024, 524288, 1, 256, 15, 1, 0, false},
    {"gpu MountainCar 2^19+64", GYMNET_ENV_MOUNTAINCAR, false, true, 0, 1024, 524352, 4, 64, 15, 1, 1, false},
    {"gpu MountainCar 10^6", GYMNET_ENV_MOUNTAINCAR, false, true, 0, 1024, 1000000, 4, 64, 15, 1, 1, false},
    {"gpu CartPole 2^19", GYMNET_ENV_CARTPOLE, false, true, 0, 1024, 524288, 1, 256, 15, 1, 0, false},
    {"gpu CartPole 3*2^18", GYMNET_ENV_CARTPOLE, false, true, 0, 1024, 786432, 4, 64, 15, 1, 1, false},
    {"gpu Acrobot 2^20", GYMNET_ENV_ACROBOT, false, true, 0, 1024, 1048576, 1, 256, 15, 4, 0, true},
    {"gpu Acrobot 2^20+1", GYMNET_ENV_ACROBOT, false, true, 0, 1024, 1048577, 1, 256, 15, 4, 0, false},
    {"gpu Acrobot 5*2^18", GYMNET_ENV_ACROBOT, false, true, 0, 1024, 1310720, 1, 256, 15, 5, 0, true},
    {"gpu CartPole64 2^20", GYMNET_ENV_CARTPOLE, true, true, 0, 1024, 1048576, 2, 256, 15, 4, 1, false},
    {"gpu CartPole64 10^6", GYMNET_ENV_CARTPOLE, true, true, 0, 1024, 1000000, 2, 256, 15, 4, 1, false},
    {"gpu CartPole64 2^20+2", GYMNET_ENV_CARTPOLE, true, true, 0, 1024, 1048578, 2, 256, 15, 1, 1, false},
    {"gpu CartPole64 3*2^18", GYMNET_ENV_CARTPOLE, true, true, 0, 1024, 786432, 2, 256, 15, 2, 1, false},
    {"gpu CartPole64 2^19", GYMNET_ENV_CARTPOLE, true, true, 0, 1024, 524288, 2, 256, 15, 1, 1, false},
    {"gpu CartPole 5*2^18", GYMNET_ENV_CARTPOLE, false, true, 0, 1024, 1310720, 4, 256, 0, 1, 1, false},
    {"gpu CartPole 2^22", GYMNET_ENV_CARTPOLE, false, true, 0, 1024, 4194304, 4, 256, 0, 1, 1, false},
    {"gpu CartPole 2^23", GYMNET_ENV_CARTPOLE, false, true, 0, 1024, 8388608, 4, 256, 12, 1, 1, false},
    {"gpu MountainCar 3*2^19", GYMNET_ENV_MOUNTAINCAR, false, true, 0, 1024, 1572864, 4, 64, 0, 1, 1, false},
    {"gpu Pendulum 2^21", GYMNET_ENV_PENDULUM, false, true, 0, 1024, 2097152, 4, 256, 12, 1, 0, false},
    {"gpu Pendulum 2^22", GYMNET_ENV_PENDULUM, false, true, 0, 1024, 4194304, 4, 256, 0, 1, 0, false},
    {"gpu CartPole64 3*2^19", GYMNET_ENV_CARTPOLE, true, true, 0, 1024, 1572864, 2, 256, 0, 1, 1, false},
    {"gpu CartPole64 2^21", GYMNET_ENV_CARTPOLE, true, true, 0, 1024, 2097152, 2, 256, 0, 1, 1, false},
    {"gpu CartPole64 2^23", GYMNET_ENV_CARTPOLE, true, true, 0, 1024, 8388608, 2, 256, 15, 1, 1, false},
    {"one generation simds 1024 n = G", GYMNET_ENV_CARTPOLE, false, true, 0, 1024, 524288, 1, 256, 15, 1, 0, false},
    {"one generation simds 1024 n = G+1", GYMNET_ENV_CARTPOLE, false, true, 0, 1024, 524289, 4, 64, 15, 1, 1, false},
    {"one generation simds 1024 n = G+1 rows 4 bytes off", GYMNET_ENV_CARTPOLE, false, true, 2, 1024, 524289, 1, 256, 15, 1, 0, false},
    {"one generation simds 1024 n = G+64", GYMNET_ENV_CARTPOLE, false, true, 0, 1024, 524352, 4, 64, 15, 1, 1, false},
    {"one generation simds 1024 MountainCar n = G", GYMNET_ENV_MOUNTAINCAR, false, false, 0, 1024, 524288, 1, 256, 15, 1, 0, false},
    {"one generation simds 1024 MountainCar n = G+64", GYMNET_ENV_MOUNTAINCAR, false, false, 0, 1024, 524352, 4, 64, 15, 1, 1, false},
    {"one generation simds 1216 n = G", GYMNET_ENV_CARTPOLE, false, true, 0, 1216, 622592, 1, 256, 15, 1, 0, false},
    {"one generation simds 1216 n = G+1", GYMNET_ENV_CARTPOLE, false, true, 0, 1216, 622593, 4, 64, 15, 1, 1, false},
    {"one generation simds 1216 n = G+1 rows 4 bytes off", GYMNET_ENV_CARTPOLE, false, true, 2, 1216, 622593, 1, 256, 15, 1, 0, false},
    {"one generation simds 1216 n = G+64", GYMNET_ENV_CARTPOLE, false, true, 0, 1216, 622656, 4, 64, 15, 1, 1, false},
    {"one generation simds 1216 MountainCar n = G", GYMNET_ENV_MOUNTAINCAR, false, false, 0, 1216, 622592, 1, 256, 15, 1, 0, false},
    {"one generation simds 1216 MountainCar n = G+64", GYMNET_ENV_MOUNTAINCAR, false, false, 0, 1216, 622656, 4, 64, 15, 1, 1, false},
    {"CartPole 5*2^18-1", GYMNET_ENV_CARTPOLE, false, true, 0, 1024, 1310719, 4, 256, 12, 1, 1, false},
    {"CartPole 5*2^18", GYMNET_ENV_CARTPOLE, false, false, 0, 1024, 1310720, 4, 256, 0, 1, 1, false},
    {"MountainCarContinuous 5*2^18-1", GYMNET_ENV_MOUNTAINCAR_CONTINUOUS, false, true, 0, 1024, 1310719, 4, 64, 15, 1, 1, false},
    {"MountainCarContinuous 5*2^18", GYMNET_ENV_MOUNTAINCAR_CONTINUOUS, false, true, 0, 1024, 1310720, 4, 64, 0, 1, 1, false},
    {"Pendulum 5*2^18", GYMNET_ENV_PENDULUM, false, true, 0, 1024, 1310720, 4, 256, 15, 1, 0, false},
    {"Pendulum 3*2^20-1", GYMNET_ENV_PENDULUM, false, true, 0, 1024, 3145727, 4, 256, 12, 1, 0, false},
    {"Pendulum 3*2^20", GYMNET_ENV_PENDULUM, false, true, 0, 1024, 3145728, 4, 256, 0, 1, 0, false},
    {"CartPole 48 MiB", GYMNET_ENV_CARTPOLE, false, true, 0, 1024, 1227601, 4, 256, 15, 1, 1, false},
    {"CartPole 48 MiB + 1 lane", GYMNET_ENV_CARTPOLE, false, true, 0, 1024, 1227602, 4, 256, 12, 1, 1, false},
    {"Pendulum 48 MiB", GYMNET_ENV_PENDULUM, false, true, 0, 1024, 1360314, 4, 256, 15, 1, 0, false},
    {"Pendulum 48 MiB + 1 lane", GYMNET_ENV_PENDULUM, false, true, 0, 1024, 1360315, 4, 256, 12, 1, 0, false},
    {"CartPole 300 MiB", GYMNET_ENV_CARTPOLE, false, true, 0, 1024, 7672507, 4, 256, 0, 1, 1, false},
    {"CartPole 300 MiB + 1 lane", GYMNET_ENV_CARTPOLE, false, true, 0, 1024, 7672508, 4, 256, 12, 1, 1, false},
    {"MountainCar 300 MiB exactly", GYMNET_ENV_MOUNTAINCAR, false, true, 0, 1024, 12582912, 4, 256, 0, 1, 1, false},
    {"MountainCar 300 MiB + 1 lane", GYMNET_ENV_MOUNTAINCAR, false, true, 0, 1024, 12582913, 4, 256, 12, 1, 1, false},
    {"Pendulum 300 MiB", GYMNET_ENV_PENDULUM, false, true, 0, 1024, 8501967, 4, 256, 0, 1, 0, false},
    {"Pendulum 300 MiB + 1 lane", GYMNET_ENV_PENDULUM, false, true, 0, 1024, 8501968, 4, 256, 12, 1, 0, false},
    {"CartPole 768 MiB", GYMNET_ENV_CARTPOLE, false, true, 0, 1024, 19641618, 4, 256, 12, 1, 1, false},
    {"CartPole 768 MiB + 1 lane", GYMNET_ENV_CARTPOLE, false, true, 0, 1024, 19641619, 1, 256, 15, 1, 0, false},
    {"MountainCar 768 MiB", GYMNET_ENV_MOUNTAINCAR, false, true, 0, 1024, 32212254, 4, 256, 12, 1, 1, false},
    {"MountainCar 768 MiB + 1 lane", GYMNET_ENV_MOUNTAINCAR, false, true, 0, 1024, 32212255, 1, 256, 15, 1, 0, false},
    {"CartPole 2^27", GYMNET_ENV_CARTPOLE, false, true, 0, 1024, 134217728, 1, 256, 15, 1, 0, false},
    {"CartPole just under 40 MiB", GYMNET_ENV_CARTPOLE, false, true, 0, 1024, 1023000, 4, 64, 15, 1, 1, false},
    {"CartPole 40 MiB reached", GYMNET_ENV_CARTPOLE, false, true, 0, 1024, 1023001, 4, 256, 15, 1, 1, false},
    {"MountainCar just under 40 MiB", GYMNET_ENV_MOUNTAINCAR, false, true, 0, 1024, 1677721, 4, 64, 0, 1, 1, false},
    {"MountainCar 40 MiB reached", GYMNET_ENV_MOUNTAINCAR, false, true, 0, 1024, 1677722, 4, 256, 0, 1, 1, false},
    {"Pendulum just under 40 MiB", GYMNET_ENV_PENDULUM, false, true, 0, 1024, 1133595, 4, 64, 15, 1, 0, false},
    {"Pendulum 40 MiB reached", GYMNET_ENV_PENDULUM, false, true, 0, 1024, 1133596, 4, 256, 15, 1, 0, false},
    {"Acrobot 2^19-1", GYMNET_ENV_ACROBOT, false, true, 0, 1024, 524287, 1, 256, 15, 1, 0, false},
    {"Acrobot 2^19", GYMNET_ENV_ACROBOT, false, true, 0, 1024, 524288, 1, 256, 15, 2, 0, true},
    {"Acrobot 2^20-1", GYMNET_ENV_ACROBOT, false, true, 0, 1024, 1048575, 1, 256, 15, 4, 0, false},
    {"Acrobot 2^20+1 no auto-reset", GYMNET_ENV_ACROBOT, false, false, 0, 1024, 1048577, 1, 256, 15, 4, 0, false},
    {"Acrobot 5*2^18 no auto-reset", GYMNET_ENV_ACROBOT, false, false, 0, 1024, 1310720, 1, 256, 15, 5, 0, true},
    {"Acrobot 11*2^17-1", GYMNET_ENV_ACROBOT, false, true, 0, 1024, 1441791, 1, 256, 15, 5, 0, false},
    {"Acrobot 11*2^17", GYMNET_ENV_ACROBOT, false, true, 0, 1024, 1441792, 1, 256, 15, 1, 0, true},
    {"Acrobot 2^23", GYMNET_ENV_ACROBOT, false, true, 0, 1024, 8388608, 1, 256, 15, 1, 0, true},
    {"CartPole64 96 MiB", GYMNET_ENV_CARTPOLE, true, true, 0, 1024, 1378949, 2, 256, 15, 1, 1, false},
    {"CartPole64 96 MiB + 1 lane", GYMNET_ENV_CARTPOLE, true, true, 0, 1024, 1378950, 2, 256, 0, 1, 1, false},
    {"CartPole64 300 MiB", GYMNET_ENV_CARTPOLE, true, true, 0, 1024, 4309216, 2, 256, 0, 1, 1, false},
    {"CartPole64 300 MiB + 1 lane", GYMNET_ENV_CARTPOLE, true, true, 0, 1024, 4309217, 2, 256, 15, 1, 1, false},
    {"CartPole64 3*2^18-1", GYMNET_ENV_CARTPOLE, true, true, 0, 1024, 786431, 2, 256, 15, 1, 1, false},
    {"CartPole64 3*2^18+1", GYMNET_ENV_CARTPOLE, true, true, 0, 1024, 786433, 2, 256, 15, 1, 1, false},
    {"CartPole64 four pairs, 1945 waves", GYMNET_ENV_CARTPOLE, true, true, 0, 1024, 995840, 2, 256, 15, 1, 1, false},
    {"CartPole64 four pairs, 1946 waves", GYMNET_ENV_CARTPOLE, true, true, 0, 1024, 995841, 2, 256, 15, 4, 1, false},
    {"CartPole64 four pairs, 2049 waves", GYMNET_ENV_CARTPOLE, true, true, 0, 1024, 1048577, 2, 256, 15, 1, 1, false},
    {"CartPole64 simds 1216 four pairs, 2310 waves", GYMNET_ENV_CARTPOLE, true, true, 0, 1216, 1182720, 2, 256, 15, 1, 1, false},
    {"CartPole64 simds 1216 four pairs, 2311 waves", GYMNET_ENV_CARTPOLE, true, true, 0, 1216, 1182721, 2, 256, 15, 4, 1, false},
    {"CartPole64 simds 1216 four pairs, 2432 waves", GYMNET_ENV_CARTPOLE, true, true, 0, 1216, 1245184, 2, 256, 15, 4, 1, false},
    {"CartPole64 simds 1216 four pairs, 2433 waves", GYMNET_ENV_CARTPOLE, true, true, 0, 1216, 1245185, 2, 256, 15, 1, 1, false},
    {"CartPole64 simds 1216 two pairs, 3465 waves", GYMNET_ENV_CARTPOLE, true, true, 0, 1216, 887040, 2, 256, 15, 1, 1, false},
    {"CartPole64 simds 1216 two pairs, 3466 waves", GYMNET_ENV_CARTPOLE, true, true, 0, 1216, 887041, 2, 256, 15, 2, 1, false},
    {"CartPole64 simds 1216 two pairs, 3648 waves", GYMNET_ENV_CARTPOLE, true, true, 0, 1216, 933888, 2, 256, 15, 2, 1, false},
    {"CartPole64 simds 1216 two pairs, 3649 waves", GYMNET_ENV_CARTPOLE, true, true, 0, 1216, 933889, 2, 256, 15, 1, 1, false},
    {"CartPole64 no auto-reset 2^20 (whole groups)", GYMNET_ENV_CARTPOLE, true, false, 0, 1024, 1048576, 2, 256, 15, 4, 1, false},
    {"CartPole64 no auto-reset 10^6 (not whole groups)", GYMNET_ENV_CARTPOLE, true, false, 0, 1024, 1000000, 2, 256, 15, 1, 1, false},
    {"CartPole64 no auto-reset 3*2^18 (whole groups)", GYMNET_ENV_CARTPOLE, true, false, 0, 1024, 786432, 2, 256, 15, 2, 1, false},
    {"CartPole64 no auto-reset 1946 waves (not whole groups)", GYMNET_ENV_CARTPOLE, true, false, 0, 1024, 995841, 2, 256, 15, 1, 1, false},
    {"CartPole 2^20 rows 4 bytes off", GYMNET_ENV_CARTPOLE, false, true, 2, 1024, 1048576, 1, 256, 15, 1, 0, false},
    {"CartPole 2^20 rows 8 bytes off", GYMNET_ENV_CARTPOLE, false, true, 1, 1024, 1048576, 1, 256, 15, 1, 0, false},
    {"Pendulum 2^22 rows 8 bytes off", GYMNET_ENV_PENDULUM, false, true, 1, 1024, 4194304, 1, 256, 0, 1, 0, false},
    {"Acrobot 2^20 aligned (lds_ok)", GYMNET_ENV_ACROBOT, false, true, 0, 1024, 1048576, 1, 256, 15, 4, 0, true},
    {"Acrobot 2^20 rows 8 bytes off", GYMNET_ENV_ACROBOT, false, true, 1, 1024, 1048576, 1, 256, 15, 4, 0, false},
    {"CartPole64 2^20 rows 8 bytes off", GYMNET_ENV_CARTPOLE, true, true, 1, 1024, 1048576, 1, 256, 15, 1, 0, false},
};

PolicyFacts facts_of(const Row &r) {
    PolicyFacts f;
    f.env_id = r.env; f.alias = kEnvFacts[r.env].alias; f.bytes_per_step = r.f64 ? 73 : kEnvFacts[r.env].bytes;
    f.f64 = r.f64; f.autoreset = r.autoreset; f.n = r.n; f.simds = r.simds;
    f.rows16 = r.align == 0; f.rows8 = r.align <= 1; f.can2_f64 = r.align == 0;
    return f;
}

}  // namespace

int main(int argc, char **argv) {
    const bool verbose = argc > 1 && std::strcmp(argv[1], "-v") == 0;
    int failed = 0, rows = 0;
    for (const Row &r : kRows) {
        const DefaultPolicy p = default_policy(facts_of(r));
        const LaunchCfg &c = p.cfg;
        bool ok = c.vec == r.vec && c.block == r.block && c.nt == r.nt && c.items == r.items && c.reset_form == r.reset_form && p.lds_ok == r.lds_ok;
        // what no rule sets: no occupancy cap, no producer / consumer form, the device's SIMD count handed through
        ok = ok && c.lds_bytes == 0 && c.lds_pipe == 0 && c.simds == r.simds;
        // the capability bits follow the alignment alone (float64: two lanes where the rows allow; float32: Acrobot's pair form from 8 bytes)
        ok = ok && p.can_vec4 == (!r.f64 && r.align == 0) && p.can_vec2 == (r.f64 ? r.align == 0 : r.align <= 1);
        ++rows;
        if (!ok || verbose)
            std::printf("%s %-58s n %-10lld got vec %d block %d nt %d items %d reset_form %d lds_ok %d | want %d %d %d %d %d %d\n", ok ? "ok  " : "FAIL", r.name,
                        (long long)r.n, c.vec, c.block, c.nt, c.items, c.reset_form, (int)p.lds_ok, r.vec, r.block, r.nt, r.items, r.reset_form, (int)r.lds_ok);
        failed += ok ? 0 : 1;
    }
    std::printf("launch policy: %d rows, %d failed\n", rows, failed);
    return failed ? 1 : 0;
}
