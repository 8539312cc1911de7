"""The recipe table of every step, rollout and resident kernel instantiation (helper module, not a conftest).

Each recipe is a dict that says how to reach ONE instantiation through the public API: env and dtype, the handle's flags, the launch
policy, the batch size and lane offset, for rollouts the action source, record mode and recorded streams — and the instantiation's
name, spelled the way step_kernels.hpp kernel_text prints it.  The table is generated from the launch-policy domain (select_step,
launch_rollout_env, launch_resident_env, capi.hip rollout_fused_ex_device); tests/test_instantiation_coverage.py pins it to the
compiled set, tests/test_gpu_instantiation_matrix.py runs every recipe against the oracle.

Batch sizes put every recipe on the places where kernels go wrong: a full unguarded workgroup, a partial last workgroup, a partial
last wave, n % V != 0 (one-shot step kernels); n % (256 * items) != 0 (step_kernel_pipe); whole 512-lane tiles with a short last
workgroup (step_kernel_lds); whole groups (strict step_kernel_pipe2) or a ragged batch (the deferred-reset float64 pipe2 forms);
n % w == 0 with a partial last workgroup (wide rollouts) or a ragged n (narrow rollouts).  Lane offsets cycle through 0, 1..3 mod 4
(the per-lane word path of action stream v2) and offsets >= 2^32."""
import itertools

# env traits (envs.hpp, cartpole64.hpp): the ones select_step / launch_rollout_env branch on
ENVS = {
    "CartPole":    dict(gym="CartPole-v1",    f64=False, alias=True,  packed=False, box=False, nvals=2, pipe_lanes=False, pipe_pairs=False, split_reset=False),
    "CartPole64":  dict(gym="CartPole-v1",    f64=True,  alias=True,  packed=False, box=False, nvals=2, pipe_lanes=False, pipe_pairs=True,  split_reset=True),
    "Pendulum":    dict(gym="Pendulum-v1",    f64=False, alias=False, packed=False, box=True,  nvals=0, pipe_lanes=False, pipe_pairs=False, split_reset=False),
    "MountainCar": dict(gym="MountainCar-v0", f64=False, alias=True,  packed=False, box=False, nvals=3, pipe_lanes=False, pipe_pairs=False, split_reset=False),
    "Acrobot":     dict(gym="Acrobot-v1",     f64=False, alias=False, packed=True,  box=False, nvals=3, pipe_lanes=True,  pipe_pairs=True,  split_reset=False),
}
NT_MASKS = (0, 12, 15)
BLOCKS = (256, 64, 128)
LANE_OFFSETS = (0, 1, 2, 3, 4102, (1 << 32) + 1, (1 << 34) + 6, (1 << 33) + 3)
LIMIT = 11                       # max_episode_steps of the recipes that truncate
LDS_TILE = 512                   # step_kernels.hpp kLdsTileMax
ROLLOUT_BLOCK = 256              # launch_rollout_env: 256 threads per workgroup


def wide_of(env):
    """step_kernels.hpp wide_of: lanes per thread of the env's wide form."""
    e = ENVS[env]
    return 2 if (e["f64"] or e["packed"]) else 4


def has_reset_form1(env, v):
    e = ENVS[env]
    return e["alias"] and not e["packed"] and v > 1


def rollout_fat_lanes(env):
    e = ENVS[env]
    return 4 if (e["f64"] and e["alias"] and not e["packed"]) else 0


def _b(v):
    return "true" if v else "false"


def _text(family, env, *targs):
    return f"{family}<{env}," + ",".join(_b(t) if isinstance(t, bool) else str(t) for t in targs) + ">"


def rollout_instantiation(env, launch_vec, n, autoreset, extras, action_source, episodes, no_overflow, reset_form, action_stride=None,
                          sstride=None):
    """Which rollout_kernel a fused rollout launches: capi.hip gymnet_vecenv_rollout_fused_ex_device's width choice, then
    step_kernels.hpp launch_rollout_env.  Every stream is assumed 16-byte aligned (the GPU test asserts it from data_ptr()).
    launch_vec: the handle's lcfg.vec; action_stride: None when the rollout reads no ring; sstride: the handle's state stride
    (the component arrays are padded to 64 lanes)."""
    e = ENVS[env]
    sstride = (n + 63) // 64 * 64 if sstride is None else sstride
    vec = launch_vec
    if vec > 1:
        def fits(w):
            return n % w == 0 and (action_stride is None or action_stride % w == 0)
        w = 2 if e["f64"] else vec
        if e["f64"] and e["alias"] and sstride % 4 == 0 and fits(4):
            vec = 4
        elif not fits(w):
            vec = 1
    fat = rollout_fat_lanes(env)
    if fat and vec == fat:
        v = fat
    elif vec in (2, 4):
        v = wide_of(env)
    else:
        v = 1
    rf = 1 if (has_reset_form1(env, v) and autoreset and reset_form == 1) else 0
    records = (2 if no_overflow else 1) if (extras and episodes) else 0
    return _text("rollout_kernel", env, v, autoreset, extras, action_source != "ring", rf, records), v


# ---- handle flag sets of the bookkeeping (EXTRAS) variants -------------------------------------------------------------------
# Any of DONE_LIST / EPISODE_STATS / FINAL_OBS or per-lane seeds selects the bookkeeping kernels (capi.hip recompute_extras).
EXTRA_SETS = (
    dict(episode_stats=True, max_episode_steps=LIMIT),
    dict(done_list=True, final_obs=True, episode_stats=True, max_episode_steps=LIMIT),
    dict(lane_seeds=True),
    dict(done_list=True),
    dict(final_obs=True, lane_seeds=True, double_buffer=True),          # (terminal observations need auto-reset: done_list instead without)
    dict(done_list=True, episode_stats=True, lane_seeds=True, max_episode_steps=LIMIT),
)
LEAN_SETS = (dict(), dict(double_buffer=True))


def _handle(env, autoreset, flags):
    if flags.get("final_obs") and not autoreset:          # GYMNET_FLAG_FINAL_OBS needs GYMNET_FLAG_AUTORESET
        flags = dict(flags, final_obs=False, done_list=True)
    h = dict(done_list=False, episode_stats=False, final_obs=False, max_episode_steps=0, double_buffer=False, lane_seeds=False,
             resident=False)
    h.update(flags)
    return dict(env=env, gym=ENVS[env]["gym"], f64=ENVS[env]["f64"], auto_reset=autoreset, **h)


def _one_shot_n(v, block):
    """Two full workgroups, then a partial one: one full wave, a partial wave of 37 threads, and (V > 1) a thread with 3 lanes."""
    return 2 * block * v + 64 * v + 37 * v + (3 if v > 1 else 0)


def step_recipes():
    out = []
    k = 0
    for env in ENVS:
        for v in sorted({1, wide_of(env)}):
            for ar, ex, nt, rf in itertools.product((False, True), (False, True), NT_MASKS, (0, 1)):
                if rf == 1 and not (ar and has_reset_form1(env, v)):
                    continue
                block = BLOCKS[k % len(BLOCKS)]
                flags = EXTRA_SETS[k % len(EXTRA_SETS)] if ex else LEAN_SETS[k % len(LEAN_SETS)]
                launch = dict(vec=v, nt=nt, block=block, sequential_lanes=1)
                if ENVS[env]["alias"]:
                    launch["reset_form"] = rf
                if env == "Acrobot":
                    launch["lds_pipe"] = 0
                out.append(dict(family="step_kernel", name=_text("step_kernel", env, v, ar, ex, nt, rf), vec=v, block=block,
                                launch=launch, n=_one_shot_n(v, block), lane_offset=LANE_OFFSETS[k % len(LANE_OFFSETS)],
                                **_handle(env, ar, flags)))
                k += 1
    # Acrobot's multi-lane forms (lean only, one lane per thread): the pipelined kernel and its producer / consumer form
    k = 0
    for items, ar in itertools.product((2, 3, 4, 5), (False, True)):
        n = 2 * 256 * items + 77                                     # not a multiple of 256 * items
        out.append(dict(family="step_kernel_pipe", name=_text("step_kernel_pipe", "Acrobot", items, ar, 15), vec=1, block=256, items=items,
                        launch=dict(vec=1, sequential_lanes=items, lds_pipe=0), n=n, lane_offset=LANE_OFFSETS[k % len(LANE_OFFSETS)],
                        **_handle("Acrobot", ar, LEAN_SETS[k % 2])))
        tiles = 2 * items + 1                                        # whole 512-lane tiles, the last workgroup short (one tile)
        out.append(dict(family="step_kernel_lds", name=_text("step_kernel_lds", "Acrobot", items, ar, 15), vec=1, block=LDS_TILE + 64,
                        items=items, launch=dict(vec=1, sequential_lanes=items, lds_pipe=1), n=tiles * LDS_TILE,
                        lane_offset=LANE_OFFSETS[(k + 3) % len(LANE_OFFSETS)], **_handle("Acrobot", ar, LEAN_SETS[(k + 1) % 2])))
        k += 1
    # lane pairs (step_kernel_pipe2): whole 2 * items * block groups, except the deferred-reset form (float64 auto-reset: any batch)
    k = 0
    for env in ("CartPole64", "Acrobot"):
        for items, ar in itertools.product((2, 3, 4), (False, True)):
            any_n = ENVS[env]["split_reset"] and ar
            for nt in ((0, 12, 15) if (any_n and items == 4) else (15,)):
                block = BLOCKS[k % len(BLOCKS)]
                group = 2 * items * block
                # (the strict form needs whole groups of 2 * items * 256 lanes whatever the block: select_step)
                n = 3 * group + 2 * 64 + 2 * 17 if any_n else 3 * (2 * items * 256)
                launch = dict(vec=2, sequential_lanes=items, block=block, nt=nt)
                if env == "Acrobot":
                    launch["lds_pipe"] = 0
                else:
                    launch["reset_form"] = 1 if ar else 0
                out.append(dict(family="step_kernel_pipe2", name=_text("step_kernel_pipe2", env, items, ar, nt), vec=2, block=block,
                                items=items, any_n=any_n, launch=launch, n=n, lane_offset=LANE_OFFSETS[k % len(LANE_OFFSETS)],
                                **_handle(env, ar, LEAN_SETS[k % 2])))
                k += 1
    return out


def rollout_recipes():
    out = []
    k = 0
    for env in ENVS:
        e = ENVS[env]
        widths = [1, wide_of(env)] + ([rollout_fat_lanes(env)] if rollout_fat_lanes(env) else [])
        for v in widths:
            for ar, ex, sample, rf, rec in itertools.product((False, True), (False, True), (False, True), (0, 1), (0, 1, 2)):
                if rf == 1 and not (ar and has_reset_form1(env, v)):
                    continue
                if rec and not ex:
                    continue
                if sample:
                    source = "epsilon_greedy" if (not e["box"] and k % 2) else "sample"
                else:
                    source = "ring"
                if ex:
                    if rec:
                        # (Pendulum's episodes end only by the time limit)
                        flags = dict(episode_stats=True, max_episode_steps=LIMIT if (k % 2 == 0 or e["box"]) else 0, lane_seeds=k % 3 == 1,
                                     done_list=k % 4 == 2, final_obs=k % 4 == 3)
                    else:
                        flags = EXTRA_SETS[k % len(EXTRA_SETS)]
                else:
                    flags = LEAN_SETS[k % 2]
                # the batch: wide forms n % v == 0 with a partial last workgroup; the narrow form a ragged n
                if v == 1:
                    n = 2 * ROLLOUT_BLOCK + 103
                    launch_vec = 1
                elif e["f64"] and v == 2:
                    n = 2 * (2 * ROLLOUT_BLOCK + 101)                 # n % 4 == 2: two lanes per thread, not the four-lane form
                    launch_vec = 2
                else:
                    n = v * (2 * ROLLOUT_BLOCK + 100)
                    launch_vec = 2 if (e["f64"] or e["packed"]) else 4
                launch = dict(vec=launch_vec)
                if e["alias"]:
                    launch["reset_form"] = rf
                stride = None if source == "sample" else n
                name, v_got = rollout_instantiation(env, launch_vec, n, ar, ex, source, rec != 0, rec == 2, rf, action_stride=stride)
                assert v_got == v, (env, v, v_got)
                # the actions taken are recorded wherever the library allows it (not on a lean ring rollout: those ARE the ring)
                rec_actions = ex or source != "ring"
                out.append(dict(family="rollout_kernel", name=name, vec=v, launch=launch, n=n, lane_offset=LANE_OFFSETS[k % len(LANE_OFFSETS)],
                                actions=source, records=("none", "overflow", "no_overflow")[rec], rec_actions=rec_actions,
                                action_stride=stride, **_handle(env, ar, flags)))
                k += 1
    return out


def resident_recipes():
    out = []
    k = 0
    for env in ENVS:
        for ar, ex in itertools.product((False, True), (False, True)):
            if ex:
                flags = (dict(episode_stats=True, max_episode_steps=LIMIT), dict(lane_seeds=True),
                         dict(episode_stats=True, lane_seeds=True, max_episode_steps=LIMIT))[k % 3]
                if env == "Pendulum" and ar and not flags.get("episode_stats"):
                    flags = dict(episode_stats=True, max_episode_steps=LIMIT, lane_seeds=True)
            else:
                flags = {}
            out.append(dict(family="resident_kernel", name=_text("resident_kernel", env, ar, ex), vec=1, launch=None,
                            n=(64, 37, 1, 50)[k % 4], lane_offset=LANE_OFFSETS[k % len(LANE_OFFSETS)], **_handle(env, ar, dict(flags, resident=True))))
            k += 1
    return out


def recipes():
    return step_recipes() + rollout_recipes() + resident_recipes()


def recipe_id(r):
    return r["name"]


# Kernels the table does not launch, with the existing tests that run them.
EXCLUDED = {
    "reset_kernel<CartPole>": "tests/test_gpu_cartpole.py (every ResetDevice / ResetWhere of a float32 CartPole handle)",
    "reset_kernel<CartPole64>": "tests/test_gpu_f64.py (every reset of a GYMNET_FLAG_F64 handle)",
    "reset_kernel<Pendulum>": "tests/test_gpu_other_envs.py (reset draws against the oracle)",
    "reset_kernel<MountainCar>": "tests/test_gpu_other_envs.py (reset draws against the oracle)",
    "reset_kernel<Acrobot>": "tests/test_gpu_other_envs.py (reset draws against the oracle)",
    "observe_kernel<Pendulum>": "tests/test_gpu_other_envs.py (SetState of a derived-observation env)",
    "observe_kernel<Acrobot>": "tests/test_gpu_other_envs.py (SetState of a derived-observation env)",
}
