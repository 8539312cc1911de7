"""The recipe table of the fused Box-actor rollout's kernels that also record the log-density of every action taken and the critic's value
(helper module, not a conftest).

actor_box_logd.hip compiles actor_box_logd_rollout_kernel<Env, AUTORESET, EXTRAS, RECORDS> in 12 forms — Pendulum and
MountainCarContinuous x auto-reset on / off x {lean, bookkeeping, bookkeeping with episode records}, the shapes of
tests/_actor_box_forms.py — and takes the policy, the log-density's two constants, the critic and both record pointers as kernel
arguments, so neither a policy nor a pointer adds a form.  Each row names one form the way the assembly demangles it and says how to reach
it through the public API: the env, the handle's auto_reset, its shape, and RolloutFusedDevice(actions="actor", rec_logd=...) under any
policy with sigma > 0.  tests/test_actor_box_logd_host.py pins the table to the compiled set; tests/test_gpu_actor_box_logd.py runs every
row under each of POLICIES."""
import _actor_box_forms as box
import _actor_box_policy_forms as pforms

ENVS, SHAPES, BOUNDS = box.ENVS, box.SHAPES, box.BOUNDS
handle_kwargs = pforms.handle_kwargs
# (head, explore, sigma) the rollout forms run under: Gaussian noise around a tanh head, and the default pair with a sigma
POLICIES = [("tanh", "gaussian", 0.3), ("clamp", "sample", 1.7)]
# ... and the act call
ACT_POLICIES = [("clamp", "gaussian", 0.5), ("tanh", "gaussian", 0.3), ("clamp", "sample", 1.7), ("tanh", "sample", 0.25)]
POISON = 7.25                                      # what the record buffers hold before the launch (a log-density may be positive)


def _b(v):
    return "true" if v else "false"


FORMS = [dict(kernel=f"actor_box_logd_rollout_kernel<{env},{_b(ar)},{_b(SHAPES[shape][0])},{_b(SHAPES[shape][1])}>", env=gym, auto_reset=ar,
              shape=shape)
         for env, gym in ENVS.items() for ar in (True, False) for shape in SHAPES]
ACT_KERNELS = ("actor_box_logd_act_kernel<2>", "actor_box_logd_act_kernel<3>")
# the actor_box_policy.hip sibling of a kernel of this unit
SIBLING = {row["kernel"]: row["kernel"].replace("actor_box_logd_rollout_kernel", "actor_box_policy_rollout_kernel") for row in FORMS}
SIBLING.update({k: k.replace("actor_box_logd_act_kernel", "actor_box_policy_act_kernel") for k in ACT_KERNELS})


def form_id(row):
    return row["kernel"]
