"""The device path's stream contract (include/gymnet_amd.h: "stream-ordered, non-blocking"; gymnet_gae_device and its kin: "capturable"), as a
table and a yardstick.  The data part — the gate arithmetic, ROWS, EXCLUDED, buffers(), the sequences and VARIANTS — imports without a GPU and is held to the
header by tests/test_stream_contract_host.py; the runner part needs torch and a device and is driven by tests/test_gpu_stream_contract.py.

The gate.  gate(stream, ms) keeps a stream busy for a known time (torch.cuda._sleep, calibrated in-process; a chain of in-place elementwise
ops where the sleep's rate cannot be trusted).  Its length is gate_ms(the host time the same sequence took in the test's reference run).

The table.  One row per device-path entry point (several where one export has forms that take different host paths):
    export      the C export the row reaches, spelled as the header spells it
    kind        which handle / buffer set the row was written for: "core", "attach", "box" (buffers(kind)) or "free" (handle-less; these run
                on a handle's stream too, over its recorded rollout)
    call        lambda (ctx, args): the call; args name the buffers (the row's defaults, overridden per sequence entry)
    outputs     the args whose buffers the call writes: poisoned on the stream ahead of the call, cloned and compared after it
    indexes     the args whose buffers hold indices, masks or weights: they must be "static" buffers, uploaded before the gate, so that a
                mis-ordered kernel reads valid but wrong data and never an out-of-range index
    blocks      None, or the sentence of the header / docstring that says the call synchronises
    capturable  True / False: whether the caller may capture the call into a graph of its own (handle calls: never, they keep host counters)

The runner.  run_gated zero-fills every buffer and uploads the static ones, synchronises, launches the gate on the caller's stream, writes the
value inputs and poisons the outputs ON that stream, issues every call with no synchronise (reading stream.query() and the host clock after
each), clones the outputs on the stream and synchronises once.  A call that ran off its stream ran before the gate ended: it read zeros where
its inputs were to come, and what it wrote was poisoned afterwards.  A call that blocks returns only after the gate has run out."""
import ctypes as C
import time

import numpy as np

# ---- the gate's arithmetic (pure) ------------------------------------------------------------------------------------------------------------
GATE_FLOOR_MS, GATE_CAP_MS, GATE_FACTOR = 50.0, 400.0, 20.0
TRIAL_CYCLES = (1_000_000, 4_000_000)        # the two calibration launches of the sleep kernel
TRIAL_OPS = (8, 32)                          # ... and of the fallback chain (in-place ops over CHAIN_ELEMENTS floats)
CHAIN_ELEMENTS = 1 << 24


def gate_ms(reference_host_ms):
    """the gate of a sequence whose reference run took reference_host_ms on the host: 20 x that, at least 50 ms, at most 400 ms"""
    return min(max(GATE_FLOOR_MS, GATE_FACTOR * float(reference_host_ms)), GATE_CAP_MS)


def derive_rate(trials):
    """[(units, measured ms)] of the two trial launches -> units per ms (the longer trial's), or None where a rate is not positive or
    the two differ by more than 2 x"""
    rates = [units / ms if ms > 0 else 0.0 for units, ms in trials]
    if min(rates) <= 0.0 or max(rates) > 2.0 * min(rates):
        return None
    return rates[-1]


def calibrate(time_sleep, time_chain):
    """time_sleep(cycles) / time_chain(ops) -> ms (event-timed on the gated stream).  ("sleep" | "chain", units per ms, the trials)"""
    trials = [(c, time_sleep(c)) for c in TRIAL_CYCLES]
    rate = derive_rate(trials)
    if rate is not None:
        return "sleep", rate, trials
    chain = [(k, time_chain(k)) for k in TRIAL_OPS]
    rate = derive_rate(chain)
    if rate is None:
        raise RuntimeError(f"the gate cannot be calibrated: sleep trials {trials}, chain trials {chain}")
    return "chain", rate, trials + chain


def units_for(rate, ms):
    return max(1, int(round(rate * ms)))


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------------
N, T, RING, HIST = 2051, 5, 2, 2             # two full workgroups of 256 threads x 4 lanes and a ragged tail of 3; ring 2
NPAD = 2052                                  # the action ring's row stride: a multiple of 4, so every row is 16-byte aligned
LIMIT = 7                                    # max_episode_steps: both done bits occur within the sequences
EP_CAP = T * N                               # episode records a rollout can leave at most
DS_ROWS = 128                                # dataset rows asked of the episode memory (16 episodes of at most 7 steps: 2/3 of each)
GATHER = 301                                 # gathered rollout-input rows
FRAME = (3, 20, 40)                          # rendered lanes, rows, pixels
SAMPLER_COUNTS = ((37, 0), (1027, (1 << 32) + 5))
POISON = {"f32": -7.25, "f64": -7.25, "i32": -0x21524111, "u8": 0xEE, "i64": -99}
NP = {"f32": np.float32, "f64": np.float64, "i32": np.int32, "u8": np.uint8, "i64": np.int64}


def _ints(lo, hi):
    return lambda rng, shape, dt: rng.integers(lo, hi, shape).astype(NP[dt])


def _normal(rng, shape, dt):
    return rng.standard_normal(shape).astype(NP[dt])


def _uniform(lo, hi):
    return lambda rng, shape, dt: rng.uniform(lo, hi, shape).astype(NP[dt])


def _rollout(prefix, obs, sdt, adt, extra=()):
    b = {f"{prefix}_obs": ((T, obs, N), sdt, "out", None), f"{prefix}_reward": ((T, N), "f32", "out", None), f"{prefix}_done": ((T, N), "u8", "out", None),
         f"{prefix}_actions": ((T, N), adt, "out", None)}
    for name in extra:
        b[f"{prefix}_{name}"] = ((T, N), "f32", "out", None)
    return b


def _episodes(prefix):
    b = {f"{prefix}_ep_{k}": ((EP_CAP,), "f32" if k == "ret" else "i32", "out", None) for k in ("step", "lane", "ret", "len")}
    b[f"{prefix}_ep_count"] = ((2,), "i32", "out", None)
    return b


def buffers(kind, sdt="f32"):
    """name -> (shape, dtype, role, generator): role "out" (written by a call), "value" (an input written on the stream under the gate)
    or "static" (indices, masks, weights: uploaded in their final form before the gate)"""
    if kind == "core":
        b = {"policy": ((N,), "i32", "value", _ints(0, 2)), "ring": ((RING, NPAD), "i32", "value", _ints(0, 2)),
             "acts_s": ((N,), "i32", "out", None), "acts_c": ((N,), "i32", "out", None), "acts_m": ((N,), "i32", "out", None),
             "action_mask": ((N, 2), "u8", "static", _ints(0, 2)), "reset_mask": ((N,), "u8", "static", _ints(0, 2)),
             "lanes": ((N,), "i32", "out", None), "lanes_count": ((1,), "i32", "out", None),
             "r_lanes": ((N,), "i32", "out", None), "r_ret": ((N,), "f32", "out", None), "r_len": ((N,), "i32", "out", None),
             "r_obs": ((N, 4), sdt, "out", None), "r_count": ((1,), "i32", "out", None),
             "packed": ((N, 4), sdt, "out", None), "frames": (FRAME, "u8", "out", None)}
        for p in ("fu", "xr", "xs", "xe", "rp"):
            b.update(_rollout(p, 4, sdt, "i32"))
            if p != "fu":
                b.update(_episodes(p))
        return b
    if kind in ("attach", "box"):
        obs, adt = (4, "i32") if kind == "attach" else (3, "f32")
        width, count, ccount = HIST * obs, actor_count(kind), critic_count(kind)
        b = {"policy": ((N,), adt, "value", _ints(0, 2) if kind == "attach" else _uniform(-2.0, 2.0)),
             "weights": ((count,), "f32", "static", _normal), "cweights": ((ccount,), "f32", "static", _normal),
             # a second set of weights, loaded first: a load that ran off its stream would leave the other set in place for the act behind it
             "weights2": ((count,), "f32", "static", _normal), "cweights2": ((ccount,), "f32", "static", _normal),
             "reset_mask": ((N,), "u8", "static", _ints(0, 2)),
             "h0": ((HIST, obs, N), "f32", "out", None), "hout": ((HIST, obs, N), "f32", "out", None),
             "value": ((N,), "f32", "out", None), "value0": ((N,), "f32", "out", None), "boot": ((N,), "f32", "out", None),
             "adv": ((T, N), "f32", "out", None), "ret": ((T, N), "f32", "out", None),
             "x": ((T, N, width), "f32", "out", None), "rows": ((GATHER,), "i64", "static", _ints(0, T * N)), "xg": ((GATHER, width), "f32", "out", None)}
        for k in (1, 2, 3):
            b[f"acts{k}"] = ((N,), adt, "out", None)
            b[f"logits{k}"] = ((N, 2 if kind == "attach" else 1), "f32", "out", None)
            b[f"logp{k}"] = ((N,), "f32", "out", None)
            b[f"value{k}"] = ((N,), "f32", "out", None)
        for p in ("rl", "rv", "rb"):
            b.update(_rollout(p, obs, "f32" if kind == "box" else sdt, adt, ("logp", "value", "boot")))
        if kind == "attach":
            b.update({"stack": ((N, 2, 20, 40), "f32", "out", None), "ds_x": ((DS_ROWS, width), "f32", "out", None), "ds_action": ((DS_ROWS,), "i32", "out", None),
                      "ds_onehot": ((DS_ROWS, 2), "f32", "out", None), "ds_reward": ((DS_ROWS,), "f32", "out", None)})
        return b
    assert kind == "free", kind
    b = {"peer_src": ((4 * N + 1,), "f32", "value", _normal), "peer_dst": ((4 * N + 1,), "f32", "out", None),
         "box_low": ((3,), "f32", "static", lambda rng, shape, dt: np.array([-1.0, -np.inf, -np.inf], np.float32)),
         "box_high": ((3,), "f32", "static", lambda rng, shape, dt: np.array([2.0, np.inf, 5.0], np.float32))}
    for k, (count, _) in enumerate(SAMPLER_COUNTS):
        b.update({f"sd{k}": ((count,), "i32", "out", None), f"sm{k}": ((count,), "i32", "out", None), f"sb{k}": ((count,), "f32", "out", None),
                  f"se{k}": ((count, 3), "f32", "out", None), f"smask{k}": ((count, 5), "u8", "static", _ints(0, 2))})
    for k, (steps, n) in enumerate(gae_shapes()):
        b.update({f"g{k}_r": ((steps, n), "f32", "value", None), f"g{k}_d": ((steps, n), "u8", "value", None), f"g{k}_v": ((steps + 1, n), "f32", "value", None),
                  f"g{k}_boot": ((steps, n), "f32", "value", None), f"g{k}_adv": ((steps, n), "f32", "out", None), f"g{k}_ret": ((steps, n), "f32", "out", None)})
    for k, (obs, hist, steps, n, m) in enumerate(inputs_shapes()):
        b.update({f"i{k}_obs": ((steps, obs, n), "f32", "value", None), f"i{k}_done": ((steps, n), "u8", "value", None), f"i{k}_h0": ((hist, obs, n), "f32", "value", None),
                  f"i{k}_hout": ((hist, obs, n), "f32", "out", None)})
        if m:
            b.update({f"i{k}_rows": ((m,), "i64", "static", _ints(0, steps * n)), f"i{k}_x": ((m, hist * obs), "f32", "out", None)})
        else:
            b[f"i{k}_x"] = ((steps, n, hist * obs), "f32", "out", None)
    return b


ACTOR_WIDTHS = {"attach": [HIST * 4, 16, 2], "box": [HIST * 3, 16, 1]}
CRITIC_WIDTHS = {"attach": [HIST * 4, 12, 1], "box": [HIST * 3, 12, 1]}


def _params(widths):
    return sum(widths[k + 1] * widths[k] + widths[k + 1] for k in range(len(widths) - 1))


def actor_count(kind):
    return _params(ACTOR_WIDTHS[kind])


def critic_count(kind):
    return _params(CRITIC_WIDTHS[kind])


def gae_shapes():
    """(T, n): n = 1030 (the one-lane form) and the smallest wide lane count (the four-lane form), each with T = 2U + 1 for its U rows in flight"""
    import _advantage_forms as aforms
    import _advantage_twin as atwin
    return ((2 * aforms.U[1] + 1, 1030), (2 * aforms.U[4] + 1, min(atwin.WIDE_NS)))


def inputs_shapes():
    """(obs_dim, history, T, n, gathered rows): the smallest dense and the smallest gathered shape test_gpu_rollout_inputs.py runs every
    form of _rollout_inputs_forms at (n = 1 and 1028 lanes, T = 6); the larger, which spans two blocks, is taken"""
    import _rollout_inputs_forms as iforms
    r = iforms.FORMS[0]["reach"]
    return ((r["obs_dim"], r["history"], 6, 1028, 0), (r["obs_dim"], r["history"], 6, 1028, 3 * 1028))


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
ROWS = {}


def row(key, export, kind, call, defaults=None, outputs=(), indexes=(), blocks=None, capturable=False):
    assert key not in ROWS, key
    ROWS[key] = {"key": key, "export": export, "kind": kind, "call": call, "defaults": dict(defaults or {}),
                 "outputs": outputs if callable(outputs) else tuple(outputs), "indexes": indexes if callable(indexes) else tuple(indexes), "blocks": blocks, "capturable": capturable}


def _fused(c, a, actions, **kw):
    p = a["p"]
    rec = dict(rec_obs=c.b[f"{p}_obs"], rec_reward=c.b[f"{p}_reward"], rec_done=c.b[f"{p}_done"])
    if kw.pop("rec_actions", True):
        rec["rec_actions"] = c.b[f"{p}_actions"]
    if kw.pop("episodes", False):
        rec["episodes"] = dict(step=c.b[f"{p}_ep_step"], lane=c.b[f"{p}_ep_lane"], ret=c.b[f"{p}_ep_ret"], length=c.b[f"{p}_ep_len"], capacity=EP_CAP,
                               count=c.b[f"{p}_ep_count"])
    for name in kw.pop("extra", ()):                           # (a Box actor's log-density goes into the buffer the Discrete rows call logp)
        rec[f"rec_{name}"] = c.b[f"{p}_{'logp' if name == 'logd' else name}"]
    ring = dict(action_stride=NPAD, ring=RING) if actions in ("ring", "epsilon_greedy") else {}
    c.env.RolloutFusedDevice(c.b["ring"] if ring else None, T, actions=actions, action_seed=77, action_tick0=900, **ring, **rec, **kw)


def _rollout_outputs(extra=(), episodes=False, actions=True):
    names = ["{p}_obs", "{p}_reward", "{p}_done"] + (["{p}_actions"] if actions else []) + [f"{{p}}_{e}" for e in extra]
    if episodes:
        names.append(("set", "{p}_ep_count", ("{p}_ep_step", "{p}_ep_lane", "{p}_ep_ret", "{p}_ep_len")))
    return names


def _p(c, name):
    return None if name is None else C.c_void_p(c.b[name].data_ptr())


# -- handle core
row("reset_device", "gymnet_vecenv_reset_device", "core", lambda c, a: c.env.ResetDevice())
row("reset_where_device[mask]", "gymnet_vecenv_reset_where_device", "core", lambda c, a: c.env.ResetWhereDevice(c.b[a["mask"]]),
    {"mask": "reset_mask"}, indexes=("mask",))
row("reset_where_device[null]", "gymnet_vecenv_reset_where_device", "core", lambda c, a: c.env.ResetWhereDevice(None))
row("step_device", "gymnet_vecenv_step_device", "core", lambda c, a: c.env.StepDevice(c.b[a["act"]]), {"act": "policy"})
row("step_repeat_device", "gymnet_vecenv_step_repeat_device", "core", lambda c, a: c.env.StepRepeatDevice(c.b[a["act"]], 2), {"act": "acts_m"})
row("rollout_device[eager]", "gymnet_vecenv_rollout_device", "core", lambda c, a: c.env.RolloutDevice(c.b["ring"], T, NPAD, RING))
row("rollout_device[graph]", "gymnet_vecenv_rollout_device", "core", lambda c, a: c.env.RolloutDevice(c.b["ring"], T, NPAD, RING))
VALIDATES = ("On a GYMNET_FLAG_VALIDATE_ACTIONS handle the calls that read the caller's Discrete actions (gymnet_vecenv_step_device, "
             "gymnet_vecenv_step_repeat_device, gymnet_vecenv_rollout_device) block: Discrete.Contains is answered by one readback before any state changes.")
row("step_device[validate]", "gymnet_vecenv_step_device", "core", lambda c, a: c.env.StepDevice(c.b["policy"]), blocks=VALIDATES)
row("step_repeat_device[validate]", "gymnet_vecenv_step_repeat_device", "core", lambda c, a: c.env.StepRepeatDevice(c.b["policy"], 1), blocks=VALIDATES)
row("rollout_device[validate]", "gymnet_vecenv_rollout_device", "core", lambda c, a: c.env.RolloutDevice(c.b["ring"], T, NPAD, RING), blocks=VALIDATES)
row("rollout_fused_device", "gymnet_vecenv_rollout_fused_device", "core",
    lambda c, a: c.check(c.lib.gymnet_vecenv_rollout_fused_device(c.env._h, _p(c, "ring"), T, NPAD, RING, C.byref(c.rollout_buffers(a["p"])))),
    {"p": "fu"}, _rollout_outputs(actions=False))
row("rollout_fused_ex_device[ring]", "gymnet_vecenv_rollout_fused_ex_device", "core", lambda c, a: _fused(c, a, "ring", episodes=True), {"p": "xr"},
    _rollout_outputs(episodes=True))
row("rollout_fused_ex_device[sample]", "gymnet_vecenv_rollout_fused_ex_device", "core", lambda c, a: _fused(c, a, "sample", episodes=True), {"p": "xs"},
    _rollout_outputs(episodes=True))
row("rollout_fused_ex_device[epsilon_greedy]", "gymnet_vecenv_rollout_fused_ex_device", "core",
    lambda c, a: _fused(c, a, "epsilon_greedy", episodes=True, epsilon=0.5), {"p": "xe"}, _rollout_outputs(episodes=True))
row("rollout_repeat_device", "gymnet_vecenv_rollout_repeat_device", "core", lambda c, a: _fused(c, a, "sample", episodes=True, repeat=1), {"p": "rp"},
    _rollout_outputs(episodes=True))
row("pack_obs_device", "gymnet_vecenv_pack_obs_device", "core", lambda c, a: c.env.PackObsDevice(c.b["packed"]), outputs=("packed",))
row("done_lanes_device", "gymnet_vecenv_done_lanes_device", "core", lambda c, a: c.env.DoneLanesDevice(c.b["lanes"], c.b["lanes_count"]),
    outputs=(("set", "lanes_count", ("lanes",)),))
row("done_records_device", "gymnet_vecenv_done_records_device", "core",
    lambda c, a: c.env.DoneRecordsDevice(c.b["r_lanes"], c.b["r_ret"], c.b["r_len"], c.b["r_obs"] if c.env._final_obs else None, N, c.b["r_count"]),
    outputs=(("set", "r_count", ("r_lanes", "r_ret", "r_len", "r_obs")),))
row("sample_actions_device", "gymnet_vecenv_sample_actions_device", "core", lambda c, a: c.env.SampleActionsDevice(c.b["acts_s"], seed=5, tick=c.round),
    outputs=("acts_s",))
row("sample_actions_masked_device", "gymnet_vecenv_sample_actions_masked_device", "core",
    lambda c, a: c.env.SampleActionsMaskedDevice(c.b["acts_m"], c.b[a["mask"]], per_lane=True, seed=6, tick=c.round), outputs=("acts_m",),
    defaults={"mask": "action_mask"}, indexes=("mask",))
row("compose_actions_device", "gymnet_vecenv_compose_actions_device", "core",
    lambda c, a: c.env.ComposeActionsDevice(c.b["policy"], 0.5, c.b["acts_c"], seed=7, tick=c.round), outputs=("acts_c",))
row("render_device", "gymnet_vecenv_render_device", "core",
    lambda c, a: c.env.RenderDevice(c.b["frames"], "gray", first_lane=N - FRAME[0], count=FRAME[0], crop=(200, 150, 200, 150), size=(FRAME[2], FRAME[1])),
    outputs=("frames",))
# -- attachments
row("pixel_stack_reset_device", "gymnet_vecenv_pixel_stack_reset_device", "attach", lambda c, a: c.stack.Reset(None if a["mask"] is None else c.b[a["mask"]]),
    {"mask": None}, outputs=("stack",), indexes=("mask",))
row("pixel_stack_push_device", "gymnet_vecenv_pixel_stack_push_device", "attach", lambda c, a: c.stack.Push(), outputs=("stack",))
row("memory_reset_device", "gymnet_vecenv_memory_reset_device", "attach",
    lambda c, a: c.memory.Reset(None if a["mask"] is None else c.b[a["mask"]], clear=a["clear"]), {"mask": None, "clear": False}, indexes=("mask",))
row("memory_push_device", "gymnet_vecenv_memory_push_device", "attach", lambda c, a: c.memory.Push(c.b[a["act"]]), {"act": "acts1"})
row("memory_push_rollout_device", "gymnet_vecenv_memory_push_rollout_device", "attach",
    lambda c, a: c.memory.PushRollout(T, c.b[a["p"] + "_obs"], c.b[a["p"] + "_actions"], c.b[a["p"] + "_reward"], c.b[a["p"] + "_done"]), {"p": "rb"})
row("memory_dataset_device", "gymnet_vecenv_memory_dataset_device", "attach",
    lambda c, a: c.check(c.lib.gymnet_vecenv_memory_dataset_device(c.env._h, c.capi.MEMORY_PARAMS, 0, 0, 0, 0, 0, 0, _p(c, "ds_x"), _p(c, "ds_action"),
                                                                   _p(c, "ds_onehot"), _p(c, "ds_reward"), DS_ROWS)),
    outputs=("ds_x", "ds_action", "ds_onehot", "ds_reward"))
row("actor_load_device", "gymnet_vecenv_actor_load_device", "attach", lambda c, a: c.actor.Load(c.b[a["w"]]), {"w": "weights"}, indexes=("w",))
row("actor_critic_load_device", "gymnet_vecenv_actor_critic_load_device", "attach", lambda c, a: c.actor.LoadCritic(c.b[a["w"]]), {"w": "cweights"},
    indexes=("w",))
row("actor_reset_device", "gymnet_vecenv_actor_reset_device", "attach", lambda c, a: c.actor.Reset(None if a["mask"] is None else c.b[a["mask"]]),
    {"mask": None}, indexes=("mask",))
row("actor_push_device", "gymnet_vecenv_actor_push_device", "attach", lambda c, a: c.actor.Push())
row("actor_history_device", "gymnet_vecenv_actor_history_device", "attach", lambda c, a: c.actor.HistoryDevice(c.b["h0"]), outputs=("h0",))
row("actor_act_device", "gymnet_vecenv_actor_act_device", "attach",
    lambda c, a: c.actor.Act(0.3, 11, c.round, out=c.b["acts1"], logits=c.b["logits1"]), outputs=("acts1", "logits1"))
row("actor_act_logp_device", "gymnet_vecenv_actor_act_logp_device", "attach",
    lambda c, a: c.actor.Act(0.3, 12, c.round, out=c.b["acts2"], logits=c.b["logits2"], logp=c.b["logp2"]), outputs=("acts2", "logits2", "logp2"))
row("actor_act_value_device", "gymnet_vecenv_actor_act_value_device", "attach",
    lambda c, a: c.actor.Act(0.3, 13, c.round, out=c.b["acts3"], logits=c.b["logits3"], logp=c.b["logp3"], value=c.b["value3"]),
    outputs=("acts3", "logits3", "logp3", "value3"))
row("actor_value_device", "gymnet_vecenv_actor_value_device", "attach", lambda c, a: c.actor.Value(c.b[a["out"]]), {"out": "value"}, outputs=("{out}",))
row("actor_boot_device", "gymnet_vecenv_actor_boot_device", "attach", lambda c, a: c.actor.Boot(c.b["boot"]), outputs=("boot",))
row("actor_box_act_device", "gymnet_vecenv_actor_box_act_device", "box",
    lambda c, a: c.actor.Act(0.6, 14, c.round, out=c.b["acts1"], logits=c.b["logits1"]), outputs=("acts1", "logits1"))
row("actor_box_act_logd_device", "gymnet_vecenv_actor_box_act_logd_device", "box",
    lambda c, a: c.actor.Act(0.6, 15, c.round, out=c.b["acts2"], logits=c.b["logits2"], logd=c.b["logp2"]), outputs=("acts2", "logits2", "logp2"))
row("rollout_fused_logp_device", "gymnet_vecenv_rollout_fused_logp_device", "attach", lambda c, a: _fused(c, a, "actor", epsilon=0.3, extra=("logp",)),
    {"p": "rl"}, _rollout_outputs(("logp",)))
row("rollout_fused_value_device", "gymnet_vecenv_rollout_fused_value_device", "attach",
    lambda c, a: _fused(c, a, "actor", epsilon=0.3, extra=("logp", "value")), {"p": "rv"}, _rollout_outputs(("logp", "value")))
row("rollout_fused_value_boot_device", "gymnet_vecenv_rollout_fused_value_boot_device", "attach",
    lambda c, a: _fused(c, a, "actor", epsilon=0.3, extra=("logp", "value", "boot")), {"p": "rb"}, _rollout_outputs(("logp", "value", "boot")))
row("rollout_fused_box_logd_device", "gymnet_vecenv_rollout_fused_box_logd_device", "box",
    lambda c, a: _fused(c, a, "actor", epsilon=0.6, extra=("logd", "value")), {"p": "rv"}, _rollout_outputs(("logp", "value")))
row("rollout_fused_box_boot_device", "gymnet_vecenv_rollout_fused_box_boot_device", "box",
    lambda c, a: _fused(c, a, "actor", epsilon=0.6, extra=("logd", "value", "boot")), {"p": "rb"}, _rollout_outputs(("logp", "value", "boot")))


# -- handle-less
def _gae(c, a):
    g = a["g"]
    if g is None:                                 # over a handle's recorded rollout
        p = a["p"]
        steps, n, names = T, N, (f"{p}_reward", f"{p}_done", f"{p}_value", "value", f"{p}_boot", "adv", "ret")
    else:
        (steps, n), names = gae_shapes()[g], (f"g{g}_r", f"g{g}_d", f"g{g}_v", None, f"g{g}_boot", f"g{g}_adv", f"g{g}_ret")
    last = _p(c, names[3]) if g is None else C.c_void_p(c.b[names[2]].data_ptr() + 4 * steps * n)
    c.check(c.lib.gymnet_gae_device(0, c.stream_ptr(), steps, n, n, _p(c, names[0]), _p(c, names[1]), _p(c, names[2]), last, _p(c, names[4]),
                                    0.99, 0.95, _p(c, names[5]), _p(c, names[6])))


def _gae_outputs(a):
    return ("adv", "ret") if a["g"] is None else (f"g{a['g']}_adv", f"g{a['g']}_ret")


def _inputs(c, a):
    k = a["i"]
    if k is None:
        p, gathered = a["p"], a["gathered"]
        obs, hist, steps, n, m = c.obs_dim, HIST, T, N, GATHER if gathered else 0
        names = (f"{p}_obs", f"{p}_done", "h0", "rows" if gathered else None, "xg" if gathered else "x", "hout")
        f64 = c.b[names[0]].element_size() == 8
    else:
        obs, hist, steps, n, m = inputs_shapes()[k]
        names, f64 = (f"i{k}_obs", f"i{k}_done", f"i{k}_h0", f"i{k}_rows" if m else None, f"i{k}_x", f"i{k}_hout"), False
    c.check(c.lib.gymnet_rollout_inputs_device(0, c.stream_ptr(), steps, n, n, obs, hist, 1 if f64 else 0, _p(c, names[0]), _p(c, names[1]), _p(c, names[2]), n,
                                               _p(c, names[3]), m, _p(c, names[4]), hist * obs, _p(c, names[5]), n))


def _inputs_outputs(a):
    if a["i"] is None:
        return ("xg" if a["gathered"] else "x", "hout")
    return (f"i{a['i']}_x", f"i{a['i']}_hout")


def _inputs_indexes(a):
    if a["i"] is None:
        return ("rows",) if a["gathered"] else ()
    return (f"i{a['i']}_rows",) if inputs_shapes()[a["i"]][4] else ()


def _sampler(which):
    def call(c, a):
        k = a["k"]
        count, off = SAMPLER_COUNTS[k]
        s, lib = c.stream_ptr(), c.lib
        if which == "discrete":
            st = lib.gymnet_sample_discrete_device(0, s, _p(c, f"sd{k}"), count, 37, 10, c.seed, off, c.round)
        elif which == "masked":
            st = lib.gymnet_sample_discrete_masked_device(0, s, _p(c, f"sm{k}"), count, 5, 3, _p(c, f"smask{k}"), 5, c.seed, off, c.round)
        elif which == "box":
            st = lib.gymnet_sample_box_device(0, s, _p(c, f"sb{k}"), count, -2.0, 2.0, c.seed, off, c.round)
        else:
            st = lib.gymnet_sample_box_elementwise_device(0, s, _p(c, f"se{k}"), count, 3, _p(c, "box_low"), _p(c, "box_high"), c.seed, off, c.round)
        c.check(st)
    return call


def _push_obs(c, a):
    dst = (C.c_void_p * 1)(c.b["peer_dst"].data_ptr())
    c.check(c.lib.gymnet_push_obs_device(0, c.stream_ptr(), _p(c, "peer_src"), dst, 1, c.b["peer_src"].numel()))


row("gae_device", "gymnet_gae_device", "free", _gae, {"g": 0, "p": "rb"}, outputs=_gae_outputs, capturable=True)
row("rollout_inputs_device[dense]", "gymnet_rollout_inputs_device", "free", _inputs, {"i": 0, "p": "rb", "gathered": False}, outputs=_inputs_outputs,
    capturable=True)
row("rollout_inputs_device[gathered]", "gymnet_rollout_inputs_device", "free", _inputs, {"i": 1, "p": "rb", "gathered": True}, outputs=_inputs_outputs,
    indexes=_inputs_indexes, capturable=True)
row("sample_discrete_device", "gymnet_sample_discrete_device", "free", _sampler("discrete"), {"k": 0}, outputs=lambda a: (f"sd{a['k']}",), capturable=True)
row("sample_discrete_masked_device", "gymnet_sample_discrete_masked_device", "free", _sampler("masked"), {"k": 0}, outputs=lambda a: (f"sm{a['k']}",),
    indexes=lambda a: (f"smask{a['k']}",), capturable=True)
row("sample_box_device", "gymnet_sample_box_device", "free", _sampler("box"), {"k": 0}, outputs=lambda a: (f"sb{a['k']}",), capturable=True)
row("sample_box_elementwise_device", "gymnet_sample_box_elementwise_device", "free", _sampler("elementwise"), {"k": 0}, outputs=lambda a: (f"se{a['k']}",),
    indexes=lambda a: ("box_low", "box_high"), capturable=True)
row("push_obs_device", "gymnet_push_obs_device", "free", _push_obs, outputs=("peer_dst",), capturable=True)

# Exports the table leaves out, each with its reason.  tests/test_stream_contract_host.py holds ROWS + EXCLUDED to the header's names exactly.
_GROUP = "a group call: it runs on streams of the group's own and needs several devices (tests/test_gpu_group*.py)"
EXCLUDED = {
    "gymnet_group_reset_device": _GROUP,
    "gymnet_group_step_device": _GROUP,
    "gymnet_group_rollout_device": _GROUP,
}


def resolve(entry):
    """a sequence entry "key" or ("key", {overrides}) -> (row, args, output specs, index buffer names)"""
    key, over = (entry, {}) if isinstance(entry, str) else entry
    r = ROWS[key]
    a = dict(r["defaults"], **over)
    outs = r["outputs"](a) if callable(r["outputs"]) else r["outputs"]

    def fmt(s):
        return s.format(**{k: v for k, v in a.items() if isinstance(v, str)}) if isinstance(s, str) else ("set", fmt(s[1]), tuple(fmt(x) for x in s[2]))
    outs = tuple(fmt(o) for o in outs)
    if callable(r["indexes"]):
        idx = tuple(r["indexes"](a))
    else:
        idx = tuple(a[k] for k in r["indexes"] if a[k] is not None)
    return r, a, outs, idx


def output_names(outs):
    names = []
    for o in outs:
        names += [o] if isinstance(o, str) else [o[1], *o[2]]
    return names


# ---- sequences: producers chained into consumers; every one opens with a step that reads an input written under the gate, AHEAD of the reset,
# so that a reset off its stream is seen too (it would run before that step and not after it) ---------------------------------------------------
def core_sequence(rollout_row, reset_null):
    seq = ["step_device", "reset_device", "sample_actions_device", "compose_actions_device", ("step_device", {"act": "acts_c"}), "done_lanes_device",
           "done_records_device", "pack_obs_device", "render_device", "sample_actions_masked_device", "step_repeat_device", "reset_where_device[mask]",
           ("step_device", {"act": "acts_s"}), "done_records_device", rollout_row, "rollout_fused_device", "rollout_fused_ex_device[ring]",
           "rollout_fused_ex_device[sample]", "rollout_fused_ex_device[epsilon_greedy]", "rollout_repeat_device", "done_lanes_device", "pack_obs_device"]
    if reset_null:
        seq += ["reset_where_device[null]", "pack_obs_device"]
    return seq


def _decision(act_row, acts, stack=True, memory=True, boot=False):
    seq = [act_row, ("step_device", {"act": acts})]
    if boot:
        seq.append("actor_boot_device")
    if stack:
        seq.append("pixel_stack_push_device")
    if memory:
        seq.append(("memory_push_device", {"act": acts}))
    return seq + ["actor_push_device"]


_TRAIN = [("gae_device", {"g": None}), ("rollout_inputs_device[dense]", {"i": None}), ("rollout_inputs_device[gathered]", {"i": None})]
# The two loads run twice over two static weight sets: load(W2), a decision and a value under W2, load(W1), the rest under W1.  A load that ran off
# its stream ran before the gate ended, so the act (the value) that follows the OTHER load on the stream would see the wrong set.
_LOAD2 = [("actor_load_device", {"w": "weights2"}), ("actor_critic_load_device", {"w": "cweights2"})]
_LOAD1 = [("actor_value_device", {"out": "value0"}), "actor_load_device", "actor_critic_load_device"]
ATTACH_SEQUENCE = (["step_device", "reset_device"] + _LOAD2 + ["actor_reset_device", "pixel_stack_reset_device", ("memory_reset_device", {"clear": True})]
                   + _decision("actor_act_device", "acts1") + _LOAD1 + _decision("actor_act_logp_device", "acts2") + _decision("actor_act_value_device", "acts3", boot=True)
                   + ["actor_history_device", "rollout_fused_value_boot_device", "memory_push_rollout_device", "actor_value_device"] + _TRAIN
                   + ["rollout_fused_logp_device", ("memory_push_rollout_device", {"p": "rl"}), "rollout_fused_value_device",
                      ("memory_reset_device", {"mask": "reset_mask"}), ("pixel_stack_reset_device", {"mask": "reset_mask"}),
                      ("actor_reset_device", {"mask": "reset_mask"}), "actor_history_device", "memory_dataset_device"])
# a float64 handle: the fused actor rollout serves float32 handles only, so the actor sequence is the unfused loop
ATTACH64_SEQUENCE = (["step_device", "reset_device"] + _LOAD2 + ["actor_reset_device", ("memory_reset_device", {"clear": True})]
                     + _decision("actor_act_device", "acts1", stack=False) + _LOAD1 + _decision("actor_act_logp_device", "acts2", stack=False)
                     + _decision("actor_act_value_device", "acts3", stack=False, boot=True) + ["actor_value_device", "actor_history_device", "memory_dataset_device"])
BOX_SEQUENCE = (["step_device", "reset_device"] + _LOAD2 + ["actor_reset_device"]
                + _decision("actor_box_act_device", "acts1", stack=False, memory=False) + _LOAD1 + _decision("actor_box_act_logd_device", "acts2", stack=False, memory=False, boot=True)
                + ["actor_history_device", "rollout_fused_box_boot_device", "actor_value_device"] + _TRAIN + ["rollout_fused_box_logd_device", "actor_history_device"])
FREE_SEQUENCE = ([(key, {"k": k}) for k in range(len(SAMPLER_COUNTS)) for key in ("sample_discrete_device", "sample_discrete_masked_device", "sample_box_device",
                                                                                   "sample_box_elementwise_device")]
                 + ["push_obs_device", "gae_device", ("gae_device", {"g": 1}), "rollout_inputs_device[dense]", "rollout_inputs_device[gathered]"])

# handle variants: constructor arguments, the launch policy set before any gate (set_launch_policy synchronises), the sequence
_BOOK = dict(auto_reset=True, done_list=True, episode_stats=True, final_obs=True, max_episode_steps=LIMIT)
VARIANTS = {
    "core-f32": dict(kind="core", env="CartPole-v1", kw=_BOOK, policy={"graph": 1}, seq=core_sequence("rollout_device[graph]", False)),
    "core-f64": dict(kind="core", env="CartPole-v1", kw=dict(_BOOK, dtype=np.float64), policy={"graph": 0}, seq=core_sequence("rollout_device[eager]", False)),
    "core-double-buffer": dict(kind="core", env="CartPole-v1", kw=dict(_BOOK, double_buffer=True), policy={"graph": 1}, seq=core_sequence("rollout_device[graph]", False)),
    # an external observation buffer, and no auto-reset: reset_where(NULL) launches here (with auto-reset it is a no-op)
    "core-ext-obs": dict(kind="core", env="CartPole-v1", kw=dict(_BOOK, auto_reset=False, final_obs=False), ext_obs=True, policy={"graph": 0},
                         seq=core_sequence("rollout_device[eager]", True)),
    # validate_actions: every call of this sequence is documented to block, so nothing after them is read as non-blocking
    "core-validate": dict(kind="core", env="CartPole-v1", kw=dict(_BOOK, validate_actions=True), policy={"graph": 0},
                          seq=["step_device[validate]", "rollout_device[validate]", "step_repeat_device[validate]"]),
    "attach-f32": dict(kind="attach", env="CartPole-v1", kw=dict(_BOOK, done_list=False), policy=None, seq=ATTACH_SEQUENCE),
    "attach-f64": dict(kind="attach", env="CartPole-v1", kw=dict(_BOOK, done_list=False, dtype=np.float64), policy=None, seq=ATTACH64_SEQUENCE),
    "box": dict(kind="box", env="Pendulum-v1", kw=dict(_BOOK, done_list=False), policy=None, seq=BOX_SEQUENCE),
    "free": dict(kind="free", env=None, kw={}, policy=None, seq=FREE_SEQUENCE),
}


# ---- the runner (torch and a device from here on) --------------------------------------------------------------------------------------------
_gates = {}


class Gate:
    """gate(stream, ms): keeps `stream` busy for ms milliseconds.  Calibrated once per process, on the first stream it is given."""

    def __init__(self, torch, stream):
        self.torch = torch
        self.scratch = None
        with torch.cuda.stream(stream):
            torch.cuda._sleep(1000)                                   # (the first launch loads the kernel)
        stream.synchronize()
        self.mode, self.rate, self.trials = calibrate(lambda c: self._timed(stream, lambda: torch.cuda._sleep(int(c))),
                                                      lambda k: self._timed(stream, lambda: self._chain(int(k))))

    def _chain(self, ops):
        if self.scratch is None:
            self.scratch = self.torch.zeros(CHAIN_ELEMENTS, dtype=self.torch.float32, device="cuda")
        for _ in range(ops):
            self.scratch.add_(1.0)

    def _timed(self, stream, launch):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            launch()
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def __call__(self, stream, ms):
        assert 0.0 < ms <= GATE_CAP_MS, ms
        units = units_for(self.rate, ms)
        with self.torch.cuda.stream(stream):
            if self.mode == "sleep":
                self.torch.cuda._sleep(units)
            else:
                self._chain(units)


def gate_for(torch, stream):
    if "gate" not in _gates:
        _gates["gate"] = Gate(torch, stream)
    return _gates["gate"]


_streams = []


def streams(torch):
    """the three torch streams of the test process (non-blocking with respect to the null stream)"""
    while len(_streams) < 3:
        _streams.append(torch.cuda.Stream())
    return _streams


class Ctx:
    """a handle (or none: the handle-less rows) of one variant, its buffers and its staged inputs.  stream None: the library's own stream,
    the arrangement the existing suite holds to the twins and the oracle"""

    def __init__(self, pkg, torch, variant, stream, seed=3):
        v = VARIANTS[variant]
        self.pkg, self.torch, self.variant, self.kind, self.stream, self.seed = pkg, torch, variant, v["kind"], stream, seed
        self.capi, self.lib = pkg._capi, pkg.load_library()
        self.round = 0
        kw = dict(v["kw"])
        sdt = "f64" if kw.get("dtype") is np.float64 else "f32"
        self.spec = buffers(self.kind, sdt)
        tdt = {"f32": torch.float32, "f64": torch.float64, "i32": torch.int32, "u8": torch.uint8, "i64": torch.int64}
        self.b = {name: torch.zeros(shape, dtype=tdt[dt], device="cuda") for name, (shape, dt, _, _) in self.spec.items()}
        rng = np.random.default_rng([seed, list(VARIANTS).index(variant)])
        self.host = {name: gen(rng, shape, dt) for name, (shape, dt, role, gen) in self.spec.items() if gen is not None}
        if self.kind == "free":
            self._free_inputs(seed)
        self.staged = {name: torch.from_numpy(np.array(a)).cuda() for name, a in self.host.items()}
        self.env = self.actor = self.stack = self.memory = None
        self.keep = []
        if v["env"] is not None:
            if v.get("ext_obs"):
                ext = torch.zeros((4, NPAD), dtype=torch.float32, device="cuda")
                self.keep.append(ext)
                kw.update(ext_obs=ext, ext_obs_stride=NPAD)
            self.env = pkg.VectorEnv(v["env"], N, seed=seed, stream=None if stream is None else stream.cuda_stream, launch_policy=v["policy"], **kw)
            self.obs_dim = self.env.ObsDim
            self.env.Reset()
            if self.kind == "attach":
                if sdt == "f32":
                    self.stack = self.env.PixelStack(depth=2, size=(40, 20), format="binary_f32", out=self.b["stack"])
                self.memory = self.env.EpisodeMemory(capacity=16, history=HIST, rollout_chunk=4)
            if self.kind in ("attach", "box"):
                import _actor_twin as atwin
                net = np.random.default_rng(seed + 100)
                self.actor = self.env.Actor(atwin.net(net, ACTOR_WIDTHS[self.kind])[2], HIST)
                self.actor.SetCritic(atwin.net(net, CRITIC_WIDTHS[self.kind])[2])
                if self.kind == "box":
                    self.actor.SetPolicy("tanh", "gaussian", 0.3)
            self.env.Sync()
        torch.cuda.synchronize()

    def _free_inputs(self, seed):
        import _advantage_twin as gtwin
        import _rollout_inputs_twin as itwin
        for k, (steps, n) in enumerate(gae_shapes()):
            c = gtwin.case(steps, n, seed)
            self.host.update({f"g{k}_r": c["r"], f"g{k}_d": c["d"], f"g{k}_v": c["v"], f"g{k}_boot": c["boot"]})
        for k, (obs, hist, steps, n, m) in enumerate(inputs_shapes()):
            c = itwin.case(obs, hist, steps, n, "bernoulli", seed=seed)
            self.host.update({f"i{k}_obs": c["rec_obs"], f"i{k}_done": c["rec_done"], f"i{k}_h0": c["history0"]})

    def check(self, status):
        self.capi.check(status)

    def stream_ptr(self):
        if self.stream is not None:
            return C.c_void_p(self.stream.cuda_stream)
        return None if self.env is None else C.c_void_p(self.env.DeviceView().stream)

    def rollout_buffers(self, p):
        rb = self.capi.RolloutBuffers(d_obs=self.b[f"{p}_obs"].data_ptr(), d_reward=self.b[f"{p}_reward"].data_ptr(), d_done=self.b[f"{p}_done"].data_ptr())
        self.keep.append(rb)
        return rb

    def close(self):
        if self.env is not None:
            self.env.Close()
            self.env = None


def _poison(torch, t):
    name = {torch.float32: "f32", torch.float64: "f64", torch.int32: "i32", torch.uint8: "u8", torch.int64: "i64"}[t.dtype]
    t.fill_(POISON[name])


def prepare(ctx):
    """step 1: zero every buffer the sequence touches, upload the static inputs in their final form"""
    for name, (_, _, role, _) in ctx.spec.items():
        if role == "static":
            ctx.b[name].copy_(ctx.staged[name])
        else:
            ctx.b[name].zero_()


def stage(ctx, seq, misplace=None):
    """step 2, on the context's current stream: the value inputs are written and every output is poisoned.  misplace = (name, stream, ms):
    that one copy is issued on another stream, which run() has put behind a gate of its own, with no event (the yardstick's own test)"""
    torch = ctx.torch
    for name, (_, _, role, _) in ctx.spec.items():
        if role != "value":
            continue
        if misplace is not None and name == misplace[0]:
            with torch.cuda.stream(misplace[1]):
                ctx.b[name].copy_(ctx.staged[name], non_blocking=True)
        else:
            ctx.b[name].copy_(ctx.staged[name], non_blocking=True)
    seen = set()
    for entry in seq:
        for name in output_names(resolve(entry)[2]):
            if name not in seen and name != "stack":             # (the stack is state a push shifts, not a buffer a call overwrites)
                seen.add(name)
                _poison(torch, ctx.b[name])


def _canonical(outs, arrays):
    """the outputs of one call as comparable bytes: a ("set", count, arrays) group becomes its first count[0] rows, sorted"""
    out = {}
    for o in outs:
        if isinstance(o, str):
            out[o] = np.ascontiguousarray(arrays[o]).view(np.uint8).reshape(-1)
            continue
        _, count, names = o
        k = int(arrays[count].view(np.uint32)[0])
        out[count] = arrays[count].view(np.uint8).reshape(-1).copy()
        k = min(k, len(arrays[names[0]]))
        if k == 0:
            out["+".join(names)] = np.zeros(0, np.uint8)
            continue
        cols = [np.ascontiguousarray(arrays[name][:k]).reshape(k, -1) for name in names]
        rows = np.concatenate([np.ascontiguousarray(col).view(np.uint8).reshape(k, -1) for col in cols], axis=1)
        order = np.lexsort(rows.T[::-1])
        out["+".join(names)] = rows[order].reshape(-1)
    return out


def issue(ctx, seq, sync_each, readings, clones, t0=0.0, query=None):
    """step 3 (and the clones of step 4, taken per call on the same stream): every call of `seq`, with no assertion in between"""
    torch = ctx.torch
    for k, entry in enumerate(seq):
        r, a, outs, _ = resolve(entry)
        r["call"](ctx, a)
        if readings is not None:
            readings.append((r["key"], bool(query()), (time.perf_counter() - t0) * 1e3))
        if sync_each:
            torch.cuda.synchronize()
        for name in output_names(outs):
            clones[f"{k:02d} {r['key']} {name}"] = ctx.b[name].clone()


def snapshot(ctx):
    """what the handle and its attachments hold once the stream has drained (blocking reads)"""
    s = {}
    if ctx.env is None:
        return s
    env = ctx.env
    s["state"], s["done"], s["reward"], s["tick"] = env.GetState(), env.GetArray("done"), env.GetArray("reward"), np.array([env.Tick], np.uint64)
    s["episode_return"], s["episode_length"] = env.GetArray("episode_return"), env.GetArray("episode_length")
    c = env.Counters()
    s["counters"] = np.array([c["lane_steps"], c["stepped_after_done"]], np.uint64)
    if ctx.actor is not None:
        s["history"] = ctx.actor.History()
    if ctx.memory is not None:
        st = ctx.memory.Stats()
        s["memory_stats"] = np.array([st[k] for k in ("kept", "ended", "admitted", "too_long")], np.int64)
        for name, a in zip(("ep_return", "ep_length", "ep_tick", "ep_lane"), ctx.memory.Episodes()):
            s["memory_" + name] = a
    return s


def run(ctx, seq, gate_length_ms=None, misplace=None):
    """One run of `seq`.  gate_length_ms None: the reference arrangement (a synchronise after every call); the host time of the calls is
    returned as the third value.  Otherwise run_gated's steps 1-4 on ctx.stream.  -> ({label: bytes}, readings, host ms)"""
    torch = ctx.torch
    ctx.round += 1
    prepare(ctx)
    torch.cuda.synchronize()
    clones, readings = {}, []
    if gate_length_ms is None:
        stage(ctx, seq)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        issue(ctx, seq, True, None, clones)
        host_ms = (time.perf_counter() - t0) * 1e3
    else:
        S = ctx.stream
        gate = gate_for(torch, S)
        if misplace is not None:
            gate(misplace[1], misplace[2])
        gate(S, gate_length_ms)
        t0 = time.perf_counter()
        with torch.cuda.stream(S):
            stage(ctx, seq, misplace)
            issue(ctx, seq, False, readings, clones, t0, S.query)
        host_ms = (time.perf_counter() - t0) * 1e3
        S.synchronize()
    torch.cuda.synchronize()
    return _results(ctx, seq, clones), readings, host_ms


def _results(ctx, seq, clones):
    arrays = {label: t.cpu().numpy() for label, t in clones.items()}
    out = {}
    for k, entry in enumerate(seq):
        r, _, outs, _ = resolve(entry)
        prefix = f"{k:02d} {r['key']} "
        mine = {label[len(prefix):]: a for label, a in arrays.items() if label.startswith(prefix)}
        for name, data in _canonical(outs, mine).items():
            out[prefix + name] = data
    for name, a in snapshot(ctx).items():
        out["after: " + name] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return out


def run_gated(ctx, seq, gate_length_ms, misplace=None):
    return run(ctx, seq, gate_length_ms, misplace)


def differences(got, want):
    """the labels whose bytes differ (or that one side lacks)"""
    bad = [k for k in want if k not in got or got[k].shape != want[k].shape or not np.array_equal(got[k], want[k])]
    return bad + [k for k in got if k not in want]


def run_interleaved(ctxs, seqs, gate_length_ms):
    """two contexts on two streams, each under its own gate, their calls issued alternately -> [results], [readings]"""
    torch = ctxs[0].torch
    for c in ctxs:
        c.round += 1
        prepare(c)
    torch.cuda.synchronize()
    clones, readings = [{} for _ in ctxs], [[] for _ in ctxs]
    gate = gate_for(torch, ctxs[0].stream)
    for c in ctxs:
        gate(c.stream, gate_length_ms)
    t0 = time.perf_counter()
    for c, seq in zip(ctxs, seqs):
        with torch.cuda.stream(c.stream):
            stage(c, seq)
    for k in range(max(len(s) for s in seqs)):
        for j, (c, seq) in enumerate(zip(ctxs, seqs)):
            if k < len(seq):
                with torch.cuda.stream(c.stream):
                    r, a, outs, _ = resolve(seq[k])
                    r["call"](c, a)
                    readings[j].append((r["key"], bool(c.stream.query()), (time.perf_counter() - t0) * 1e3))
                    for name in output_names(outs):
                        clones[j][f"{k:02d} {r['key']} {name}"] = c.b[name].clone()
    for c in ctxs:
        c.stream.synchronize()
    torch.cuda.synchronize()
    return [_results(c, seq, cl) for c, seq, cl in zip(ctxs, seqs, clones)], readings


def record(line):
    """a line of the run's record: calibration, gates, readings, verdicts (pytest -s shows them; profiles/stream_contract.txt keeps one run's)"""
    print(line)
