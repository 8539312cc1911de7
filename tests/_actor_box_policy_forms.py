"""The recipe table of the fused Box-actor rollout's kernels under a policy other than the default (helper module, not a conftest).

actor_box_policy.hip compiles actor_box_policy_rollout_kernel<Env, AUTORESET, EXTRAS, RECORDS> in 12 forms — Pendulum and
MountainCarContinuous x auto-reset on / off x {lean, bookkeeping, bookkeeping with episode records}, the shapes of
tests/_actor_box_forms.py — and takes head, explore and sigma as kernel arguments, so a policy adds no form.  Each row names one form the
way the assembly demangles it and says how to reach it through the public API: the env, the handle's auto_reset, its shape, and any
policy but ("clamp", "sample") set on the handle's actor (Actor.SetPolicy): the default runs actor_box.hip's kernel of the same shape
instead.  tests/test_actor_box_policy_host.py pins the table to the compiled set; tests/test_gpu_actor_box_policy.py runs every row
under each of POLICIES."""
import _actor_box_forms as box

ENVS, SHAPES = box.ENVS, box.SHAPES
# (head, explore, sigma): every non-default combination of the two switches
POLICIES = [("tanh", "gaussian", 0.5), ("clamp", "gaussian", 0.5), ("tanh", "sample", 0.0)]


def _b(v):
    return "true" if v else "false"


FORMS = [dict(kernel=f"actor_box_policy_rollout_kernel<{env},{_b(ar)},{_b(SHAPES[shape][0])},{_b(SHAPES[shape][1])}>", env=gym, auto_reset=ar,
              shape=shape)
         for env, gym in ENVS.items() for ar in (True, False) for shape in SHAPES]
ACT_KERNELS = ("actor_box_policy_act_kernel<2>", "actor_box_policy_act_kernel<3>")


def form_id(row):
    return row["kernel"]


def handle_kwargs(row, limit):
    kw = dict(auto_reset=row["auto_reset"])
    if row["shape"] != "lean":
        kw.update(episode_stats=True, max_episode_steps=limit)
    return kw
