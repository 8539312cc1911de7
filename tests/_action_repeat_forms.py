"""One row per compiled repeat_rollout_kernel<Env, AUTORESET, EXTRAS, SAMPLE, RECORDS> of gym.net_amd/csrc/action_repeat.hip (helper module,
not a conftest): the kernel's name as tools/kernel_resources.py prints it -> the env, dtype, handle flags and action source that reach it
through VectorEnv.RolloutFusedDevice(..., repeat > 0).  tests/test_action_repeat_host.py holds the table to the unit's compiled kernel set;
tests/test_gpu_action_repeat.py runs every row."""
import numpy as np

# kernel env name -> (gym id, dtype)
ENVS = {"CartPole": ("CartPole-v1", np.float32), "CartPole64": ("CartPole-v1", np.float64), "Pendulum": ("Pendulum-v1", np.float32),
        "MountainCar": ("MountainCar-v0", np.float32), "MountainCarContinuous": ("MountainCarContinuous-v0", np.float32),
        "Acrobot": ("Acrobot-v1", np.float32)}
# shape -> (EXTRAS, RECORDS): a lean handle; a bookkeeping handle (episode_stats + max_episode_steps); the same with episode records asked for
SHAPES = {"lean": (False, False), "bookkeeping": (True, False), "records": (True, True)}
# action source -> SAMPLE ("ring" reads d_actions[d % ring]; "sample" draws in the kernel; "epsilon_greedy" is Discrete-only and runs the
# SAMPLE kernel too: the GPU test adds it to the Discrete rows)
SOURCES = {"ring": False, "sample": True}


def _b(v):
    return "true" if v else "false"


FORMS = [{"kernel": f"repeat_rollout_kernel<{env},{_b(ar)},{_b(SHAPES[shape][0])},{_b(SOURCES[src])},{_b(SHAPES[shape][1])}>",
          "env": ENVS[env][0], "dtype": ENVS[env][1], "name": env, "auto_reset": ar, "shape": shape, "actions": src}
         for env in ENVS for ar in (True, False) for shape in SHAPES for src in SOURCES]
