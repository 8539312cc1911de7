// env_mountaincar_continuous.hip — MountainCarContinuous's launcher table (step_kernels.hpp launchers_of), which instantiates its step /
// rollout / reset kernels: MountainCarContinuous-v0 (absent from the reference; upstream gym).  One translation unit per env so the build
// compiles them side by side.
#include "step_kernels.hpp"

#include "envs.hpp"

namespace gymnet {
const EnvLaunchers<float> &mountaincar_continuous_launchers() {
    static const EnvLaunchers<float> table = launchers_of<MountainCarContinuous>();
    return table;
}
}
