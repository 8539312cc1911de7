// env_cartpole64.hip — CartPole64's launcher table (step_kernels.hpp launchers_of), which instantiates its step / rollout / reset kernels:
// GYMNET_FLAG_F64 — CartPole in the reference's own binary64 arithmetic (CartPoleEnv.cs:141-166,185).  One translation unit per env so the build compiles them side by side.
#include "step_kernels.hpp"

#include "cartpole64.hpp"

namespace gymnet {
const EnvLaunchers<double> &cartpole64_launchers() {
    static const EnvLaunchers<double> table = launchers_of<CartPole64>();
    return table;
}
}
