"""The recipe table of MountainCarContinuous's step, rollout and resident kernel instantiations (helper module, not a conftest).

The env's translation unit (csrc/env_mountaincar_continuous.hip) is the first to instantiate the skeleton for a Box action together with
termination, so its table is generated here, in the shape of tests/_instantiation_matrix.py (whose table covers the five older units and
is pinned to exactly their kernels) and with its helpers.  tests/test_mountaincar_continuous_host.py pins this table to the unit's
compiled kernel set; tests/test_gpu_mountaincar_continuous.py runs every recipe against the float32 twin, bit for bit.

The env's traits, as select_step / launch_rollout_env see them: the observation IS the state (the wave-compacted reset exists for the
four-lane forms), no packed form, no multi-lane forms, Box actions (the rollout draws Box.Sample(); epsilon-greedy is refused)."""
import itertools

import _instantiation_matrix as M

ENV = "MountainCarContinuous"
TRAITS = dict(gym="MountainCarContinuous-v0", f64=False, alias=True, packed=False, box=True, nvals=0, pipe_lanes=False, pipe_pairs=False,
              split_reset=False)
WIDE = 4                                                  # step_kernels.hpp wide_of: four floats per thread


def has_reset_form1(v):
    return v > 1                                          # alias, unpacked: step_kernels.hpp has_reset_form1


def rollout_instantiation(launch_vec, n, autoreset, extras, action_source, episodes, no_overflow, reset_form, action_stride=None):
    """Which rollout_kernel a fused rollout launches (M.rollout_instantiation's rules for a float32, unpacked env): the handle's lane width
    if n and the action stride are whole groups of it, else one lane per thread."""
    v = launch_vec
    if v > 1 and not (n % v == 0 and (action_stride is None or action_stride % v == 0)):
        v = 1
    v = WIDE if v in (2, 4) else 1
    rf = 1 if (has_reset_form1(v) and autoreset and reset_form == 1) else 0
    records = (2 if no_overflow else 1) if (extras and episodes) else 0
    return M._text("rollout_kernel", ENV, v, autoreset, extras, action_source != "ring", rf, records), v


def _handle(autoreset, flags):
    if flags.get("final_obs") and not autoreset:          # GYMNET_FLAG_FINAL_OBS needs GYMNET_FLAG_AUTORESET
        flags = dict(flags, final_obs=False, done_list=True)
    h = dict(done_list=False, episode_stats=False, final_obs=False, max_episode_steps=0, double_buffer=False, lane_seeds=False,
             resident=False)
    h.update(flags)
    return dict(env=ENV, gym=TRAITS["gym"], f64=False, auto_reset=autoreset, **h)


def step_recipes():
    out = []
    k = 0
    for v in (1, WIDE):
        for ar, ex, nt, rf in itertools.product((False, True), (False, True), M.NT_MASKS, (0, 1)):
            if rf == 1 and not (ar and has_reset_form1(v)):
                continue
            block = M.BLOCKS[k % len(M.BLOCKS)]
            flags = M.EXTRA_SETS[k % len(M.EXTRA_SETS)] if ex else M.LEAN_SETS[k % len(M.LEAN_SETS)]
            launch = dict(vec=v, nt=nt, block=block, sequential_lanes=1, reset_form=rf)
            out.append(dict(family="step_kernel", name=M._text("step_kernel", ENV, v, ar, ex, nt, rf), vec=v, block=block, launch=launch,
                            n=M._one_shot_n(v, block), lane_offset=M.LANE_OFFSETS[k % len(M.LANE_OFFSETS)], **_handle(ar, flags)))
            k += 1
    return out


def rollout_recipes():
    out = []
    k = 0
    for v in (1, WIDE):
        for ar, ex, sample, rf, rec in itertools.product((False, True), (False, True), (False, True), (0, 1), (0, 1, 2)):
            if rf == 1 and not (ar and has_reset_form1(v)):
                continue
            if rec and not ex:
                continue
            source = "sample" if sample else "ring"
            if ex:
                if rec:
                    flags = dict(episode_stats=True, max_episode_steps=M.LIMIT if k % 2 == 0 else 0, lane_seeds=k % 3 == 1,
                                 done_list=k % 4 == 2, final_obs=k % 4 == 3)
                else:
                    flags = M.EXTRA_SETS[k % len(M.EXTRA_SETS)]
            else:
                flags = M.LEAN_SETS[k % 2]
            # the batch: the wide form n % 4 == 0 with a partial last workgroup; the narrow form a ragged n
            n = 2 * M.ROLLOUT_BLOCK + 103 if v == 1 else v * (2 * M.ROLLOUT_BLOCK + 100)
            launch = dict(vec=1 if v == 1 else 4, reset_form=rf)
            stride = None if source == "sample" else n
            name, v_got = rollout_instantiation(launch["vec"], n, ar, ex, source, rec != 0, rec == 2, rf, action_stride=stride)
            assert v_got == v, (v, v_got)
            out.append(dict(family="rollout_kernel", name=name, vec=v, launch=launch, n=n, lane_offset=M.LANE_OFFSETS[k % len(M.LANE_OFFSETS)],
                            actions=source, records=("none", "overflow", "no_overflow")[rec], rec_actions=ex or source != "ring",
                            action_stride=stride, **_handle(ar, flags)))
            k += 1
    return out


def resident_recipes():
    # (lane offsets 0, 1, 2^34 + 6, 3: every residue mod 4 and one beyond 2^32)
    out = []
    k = 0
    for ar, ex in itertools.product((False, True), (False, True)):
        flags = (dict(episode_stats=True, max_episode_steps=M.LIMIT), dict(lane_seeds=True),
                 dict(episode_stats=True, lane_seeds=True, max_episode_steps=M.LIMIT))[k % 3] if ex else {}
        out.append(dict(family="resident_kernel", name=M._text("resident_kernel", ENV, ar, ex), vec=1, launch=None, n=(64, 37, 1, 50)[k % 4],
                        lane_offset=M.LANE_OFFSETS[(0, 1, 6, 3)[k]], **_handle(ar, dict(flags, resident=True))))
        k += 1
    return out


def recipes():
    return step_recipes() + rollout_recipes() + resident_recipes()


# Kernels the table does not launch, with the tests that run them.
EXCLUDED = {
    "reset_kernel<MountainCarContinuous>": "tests/test_gpu_mountaincar_continuous.py (every ResetDevice / Reset, checked against the reset twin)",
}
