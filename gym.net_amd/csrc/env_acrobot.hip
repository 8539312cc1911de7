// env_acrobot.hip — Acrobot's launcher table (step_kernels.hpp launchers_of), which instantiates its step / rollout / reset kernels:
// Acrobot-v1 (absent from the reference; upstream gym).  One translation unit per env so the build compiles them side by side.
#include "step_kernels.hpp"

#include "envs.hpp"

namespace gymnet {
const EnvLaunchers<float> &acrobot_launchers() {
    static const EnvLaunchers<float> table = launchers_of<Acrobot>();
    return table;
}
}
