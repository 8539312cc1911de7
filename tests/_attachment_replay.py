"""The handle's attachments on the CPU (helper module, not a conftest): AttachedModel stands on tests/_handle_replay.py HandleModel and
carries what the actor, the pixel stack and the episode memory hold between calls —

  the actor's history (tests/_actor_twin.py History) and its ring slot, its weights and its critic's;
  the pixel stack (tests/_pixel_stack_model.py) and the episode memory (tests/_episode_memory_model.py);
  the actor's and the memory's staleness state, worded as include/gymnet_amd.h words it (Gate): how many vector decisions and step
  launches ran since the attachment's last config / reset / push / actor rollout, and whether one of the calls the header lists as
  leaving it stale came in between — a reset of the handle that launches, seed, seed_lanes, set_tick, set_state, per-lane keys through
  set_array, a restored checkpoint.  act / value need none of either; a push / boot exactly one decision in one launch; a rollout push
  of k steps exactly k decisions in one launch.  A host-boundary step the resident kernel serves is a decision but no step launch.

The model never reads a handle, with one exception: the GRAY8 frame of the current observation, which the caller renders with
RenderDevice on the handle under test and passes in (the raster has its own twin tests, tests/test_gpu_raster_geometry.py; here only the
stack's rules are under test).

CONFIGS are the configurations tests/test_gpu_attachment_sequences.py opens; apply() runs one operation of tests/_attachment_sequences.py
on the model and returns (accepted, what it recorded)."""
import numpy as np

import _actor_boot_cases as boot_cases
import _actor_box_forms as box_forms
import _actor_logp_twin as logp_twin
import _actor_softmax_twin as soft_twin
import _actor_twin as twin
import _episode_memory_model as mem_model
import _handle_replay as H
import _pixel_stack_model as stack_model

F32 = np.float32
CROP, SIZE = (200, 150, 200, 150), (16, 8)

# small on purpose: 259 = four waves and three lanes (a guarded tail of the four-lane forms), 130 = two waves and two lanes; ext: a
# caller-owned observation buffer of stride n + 12 (a pair of them on a double-buffered handle); critic / boot where the configuration has
# them; explore: a Discrete actor's exploration setting; keys: per-lane Philox keys installed in the prologue.  A Box actor runs under the
# policy ("clamp", "sample", 0), set explicitly: it is the one policy whose actions a CPU twin reproduces bit for bit
# (tests/_actor_box_forms.py compose), which a model that steps with its own actions needs — the tanh head and the Gaussian draw are held
# to a bound in tests/test_gpu_actor_box_policy.py, not to bits
CONFIGS = {
    "P": dict(H._cfg("CartPole", 259, auto_reset=True, double_buffer=True, episode_stats=True, final_obs=True, max_episode_steps=9,
                     lane_offset=(1 << 32) + 5), ext=False, critic=True, stack=True, memory=True, max_length=0),
    "Q": dict(H._cfg("CartPole", 259, episode_stats=True, done_list=True), ext=True, critic=False, stack=True, memory=True, max_length=12),
    "S": dict(H._cfg("CartPole64", 130, auto_reset=True, double_buffer=True, done_list=True, episode_stats=True), ext=False, critic=True,
              stack=True, memory=True, max_length=12),
    "T": dict(H._cfg("Pendulum", 259, auto_reset=True, double_buffer=True, episode_stats=True, final_obs=True, max_episode_steps=7), ext=True,
              critic=True, stack=False, memory=True, max_length=0),
    "U": dict(H._cfg("Acrobot", 130, done_list=True, episode_stats=True), ext=False, critic=False, stack=False, memory=True, max_length=12,
              keys=True, explore=("softmax", 0.5)),
    "R": dict(H._cfg("CartPole", 7, auto_reset=True, episode_stats=True, resident=True, share=0.6), ext=False, critic=False, stack=False,
              memory=False, max_length=0),
}
for _c in CONFIGS.values():
    _c.setdefault("keys", False)
    _c.setdefault("explore", ("uniform", 1.0))
    _c["box"] = H.M.ENVS[_c["env"]]["box"]
BOX_POLICY = ("clamp", "sample", 0.0)


def outputs_of(c):
    """the width of the actor's last layer: the Discrete space's n, or the Box action's one dimension"""
    return 1 if c["box"] else H.M.ENVS[c["env"]]["nvals"]

# the parameter sets a (re-)config alternates between
VARIANTS = {"actor": (dict(S=2, hidden=8), dict(S=3, hidden=5)), "stack": (dict(depth=2), dict(depth=3)),
            "memory": (dict(capacity=5, history=2, chunk=4), dict(capacity=3, history=3, chunk=2))}
HANDLE_KINDS = ("step", "rollout", "decision", "reset", "reset_where", "seed", "set_lane_seeds", "set_tick", "set_state", "set_array", "checkpoint", "restore")
ATTACHMENT_KINDS = ("act", "actor_push", "actor_reset", "actor_step", "actor_load", "actor_rollout", "boot", "value", "stack_push",
                    "stack_reset", "mem_push", "mem_reset", "mem_rollout", "reconfig")
# what a refused call's message starts with
PREFIX = {"act": "the actor's history is stale", "value": "the actor's history is stale", "actor_step": "the actor's history is stale",
          "actor_rollout": "the actor's history is stale", "actor_push": "an actor push needs exactly one vector step",
          "boot": "an actor boot needs exactly one vector step", "mem_push": "a push needs exactly one vector step",
          "mem_rollout": "a push needs exactly one vector step"}


def kinds_of(c):
    """the attachment operation kinds configuration c takes"""
    out = {"act", "actor_push", "actor_reset", "actor_step", "actor_load", "reconfig"}
    if not c["f64"]:                                # (the header says which calls a float64 handle's actor serves: no fused actor rollout)
        out.add("actor_rollout")
    if c["critic"]:
        out |= {"value"} | ({"boot"} if c["max_episode_steps"] else set())
    if c["stack"]:
        out |= {"stack_push", "stack_reset"}
    if c["memory"]:
        out |= {"mem_push", "mem_reset", "mem_rollout"}
    return out


def net_of(seed, S, hidden, out, O=4):
    return twin.net(np.random.default_rng([int(seed), S, hidden, out, O]), [S * O, hidden, out], scale=2.0)


class Gate:
    """An attachment's staleness state in the header's words."""

    def __init__(self):
        self.decisions = self.launches = 0
        self.void = False

    def stepped(self, decisions, launches):
        self.decisions += decisions
        self.launches += launches

    def current(self):
        return not self.void and (self.decisions, self.launches) == (0, 0)

    def one_launch_of(self, k):
        return not self.void and k >= 1 and (self.decisions, self.launches) == (k, 1)


def advance(gates, op, c):
    """What a handle operation does to every gate (pure: the sequence generator and the host test use it without a model)."""
    k = op["kind"]
    if k in ("step", "decision"):
        served = c["resident"] and k == "step" and op["path"] in ("Step", "StepInt", "StepInto")
        for g in gates:
            g.stepped(1, 0 if served else 1)
    elif k == "rollout":
        for g in gates:
            g.stepped(op["T"], 1 if op["path"] == "fused" else op["T"])
    elif k == "reset_where" and op["mask"] is None and c["auto_reset"]:
        pass                                        # the documented no-op: nothing goes stale
    elif k in ("reset", "reset_where", "seed", "set_lane_seeds", "set_tick", "set_state", "restore"):
        for g in gates:
            g.void = True


class AttachedModel(H.HandleModel):
    def __init__(self, oracle, c):
        super().__init__(oracle, c)
        self.cfg = c
        self.actor = self.critic = self.hist = self.stack = self.memory = None
        self.slot = 0
        self.gate = {"actor": Gate(), "memory": Gate()}
        self.variant = {"actor": 0, "stack": 0, "memory": 0}
        self.last_a = None                          # the actions of the last step taken (what a memory push is handed)

    # -- configuration -----------------------------------------------------------------------------------------------------------
    def obs_rows(self):
        return np.ascontiguousarray(self.obs.T)

    def config(self, which, variant, gray=None):
        v = VARIANTS[which][variant]
        self.variant[which] = variant
        if which == "actor":
            self.S = v["S"]
            self.actor = net_of(1, v["S"], v["hidden"], outputs_of(self.cfg), H.obs_dim(self.cfg))
            self.critic = net_of(2, v["S"], v["hidden"], 1, H.obs_dim(self.cfg)) if self.cfg["critic"] else None
            self.hist, self.slot = twin.History(self.obs_rows(), v["S"]), 0
            self.gate["actor"] = Gate()
        elif which == "stack":
            self.stack = stack_model.PixelStackModel(gray, v["depth"])
        else:
            limit = self.cfg["max_length"] or self.cfg["max_episode_steps"]
            self.memory = mem_model.EpisodeMemoryModel(self.obs_rows(), v["capacity"], limit, v["history"], autoreset=self.cfg["auto_reset"])
            self.gate["memory"] = Gate()

    # -- the actor ---------------------------------------------------------------------------------------------------------------
    def act(self, eps, seed, tick):
        """dict(actions, logits, logp bits or None, value or None) of one act call over the history"""
        w, flat, _ = self.actor
        x = np.ascontiguousarray(self.hist.x())
        logits = twin.forward(w, flat, x)[0]
        wa, wb = soft_twin.words(seed, self.lo, tick, self.n)
        if self.cfg["box"]:
            low, high = box_forms.BOUNDS[self.cfg["gym"]]
            actions, _ = box_forms.compose(logits[:, 0], wa, wb, eps, low, high)
            out = dict(actions=actions, logits=logits, logp=None, value=None)
        else:
            explore, tau = self.cfg["explore"]
            actions, _, _ = soft_twin.act(logits, wa, wb, eps, explore, tau)
            out = dict(actions=actions.astype(np.int32), logits=logits, logp=logp_twin.logp(logits, actions, tau), value=None)
        if self.critic is not None:
            out["value"] = self.value()
        return out

    def value(self):
        w, flat, _ = self.critic
        return twin.forward(w, flat, np.ascontiguousarray(self.hist.x()))[0][:, 0]

    def boot(self):
        term = self.final.T if self.cfg["auto_reset"] else self.obs.T
        return boot_cases.want_boot(self.critic, self.hist.h, term, self.done)

    def actor_push(self):
        self.hist.push(self.obs_rows(), self.done)
        self.slot = (self.slot + 1) % self.S
        self.gate["actor"] = Gate()

    def actor_reset(self, mask):
        self.hist.reset(self.obs_rows(), mask)
        self.gate["actor"] = Gate()

    # -- the stack and the memory ------------------------------------------------------------------------------------------------
    def stack_push(self, gray):
        self.stack.push(gray, self.done if self.cfg["auto_reset"] else None)

    def mem_push(self, actions):
        ended = self.memory.push(actions, self.reward, self.done, self.obs_rows(), self.tick)
        self.gate["memory"] = Gate()
        return ended

    def mem_reset(self, mask, clear):
        self.memory.reset(self.obs_rows(), mask, clear)
        self.gate["memory"] = Gate()


def apply(m, op, slots, gray=None):
    """One operation on the model.  gray: the handle's rendered frame of the current observation where the operation feeds the stack
    (stack_push, stack_reset, reconfig of the stack) — rendered AFTER the handle took the operation.  Returns (accepted, record):
    accepted False means the library must refuse the call (and, for mem_rollout, that it does so after its launch has run)."""
    k, c = op["kind"], m.cfg
    gates = list(m.gate.values())
    if k in HANDLE_KINDS:
        if k == "set_tick" and op["value"] == "same":
            op = dict(op, value=m.tick)
        rec = H.apply(m, op, slots)
        advance(gates, op, c)
        if k in ("step", "decision"):
            m.last_a = np.asarray(rec["a"])
        elif k == "rollout":
            m.last_a = np.asarray(rec[-1]["a"])
        return True, rec
    if k == "reconfig":
        m.config(op["which"], op["variant"], gray)
        return True, None
    if k == "act":
        return (True, m.act(op["eps"], op["seed"], op["tick"])) if m.gate["actor"].current() else (False, None)
    if k == "value":
        return (True, m.value()) if m.gate["actor"].current() else (False, None)
    if k == "boot":
        return (True, m.boot()) if m.gate["actor"].one_launch_of(1) else (False, None)
    if k == "actor_push":
        if not m.gate["actor"].one_launch_of(1):
            return False, None
        m.actor_push()
        return True, None
    if k == "actor_reset":
        m.actor_reset(op["mask"])
        return True, None
    if k == "actor_load":
        m.actor = net_of(op["net_seed"], m.S, VARIANTS["actor"][m.variant["actor"]]["hidden"], outputs_of(c), H.obs_dim(c))
        return True, None
    if k in ("actor_step", "actor_rollout"):
        if not m.gate["actor"].current():
            return False, None
        T = 1 if k == "actor_step" else op["T"]
        recs = []
        for t in range(T):
            a = m.act(op["eps"], op["seed"], op["tick"] + t)
            rec = m.step(a["actions"])
            m.hist.push(m.obs_rows(), m.done)
            recs.append(dict(rec, act=a))
        m.slot = (m.slot + T) % m.S
        m.last_a = recs[-1]["a"]
        for g in gates:
            g.stepped(T, 1)
        m.gate["actor"] = Gate()
        return True, recs
    if k == "stack_push":
        m.stack_push(gray)
        return True, None
    if k == "stack_reset":
        m.stack.reset(gray, op["mask"])
        return True, None
    if k == "mem_push":
        if not m.gate["memory"].one_launch_of(1):
            return False, None
        return True, m.mem_push(m.last_a)
    if k == "mem_reset":
        m.mem_reset(op["mask"], op["clear"])
        return True, None
    if k == "mem_rollout":
        ok = m.gate["memory"].current()
        ring, ended = np.asarray(op["ring"]), []
        for t in range(op["T"]):
            m.step(ring[t])
            if ok:
                ended.append(m.memory.push(ring[t], m.reward, m.done, m.obs_rows(), m.tick))
        m.last_a = ring[op["T"] - 1]
        for g in gates:
            g.stepped(op["T"], 1)
        if ok:
            m.gate["memory"] = Gate()
        return ok, ended
    raise KeyError(k)
