// env_cartpole.hip — CartPole's launcher table (step_kernels.hpp launchers_of), which instantiates its step / rollout / reset kernels:
// CartPole-v1 in float32 (CartPoleEnv.cs:24-67,137-186), the structure-of-arrays hot path.  One translation unit per env so the build compiles them side by side.
#include "step_kernels.hpp"

#include "envs.hpp"

namespace gymnet {
const EnvLaunchers<float> &cartpole_launchers() {
    static const EnvLaunchers<float> table = launchers_of<CartPole>();
    return table;
}
}
