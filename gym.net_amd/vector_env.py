"""VectorEnv — the batched replacement for Gym.NET's VecEnv / Env hot path, over the C ABI.

Mirrors (paths relative to the Gym.NET tree):
  IVecEnv / VecEnv     src/Gym/Envs/IVecEnv.cs:8-19, src/Gym/Envs/VecEnv.cs:12-93
  VecEnvWrapper        src/Gym/Envs/VecEnvWrapper.cs:9-30      (the sequential map this replaces)
  IEnv / Env           src/Gym/Envs/IEnv.cs:11-22, src/Gym/Envs/Env.cs:13-41
  CartPoleEnv          src/Gym.Environments/Envs/Classic/CartPoleEnv.cs:43-67,137-198

Same member names (Reset, Step, StepAsync, Seed, Close, ActionSpace, ObservationSpace, Metadata,
RewardRange, NumberOfEnvironments), same argument meaning, same error behaviour.  Deviations, all
forced by scale: results are ARRAYS — Reset() returns one ndarray [N, D] instead of
NDArray[N], Step() returns a BatchStep whose items are the reference's Step records — and Step()
also accepts one action PER LANE.  `Environments` is empty: 2^20 IEnv objects are never built.

Everything here is a thin shim over libgymnet_amd.so: all compute happens in HIP kernels.  NDArray
is numpy.ndarray on this side of the boundary.
"""
import ctypes as C
import enum

import numpy as np

from . import _capi as capi
from .errors import AlreadySteppingError, NotSteppingError
from .spaces import Box, Discrete
from .step import Step


def _ptr(x):
    """Device pointer from an int, a ctypes pointer or anything with .data_ptr() (torch tensor)."""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    if isinstance(x, C.c_void_p):
        return x
    return C.c_void_p(int(x))


def _host(a):
    return a.ctypes.data_as(C.c_void_p)


def _repeat(repeat):
    """`repeat` skipped frames per decision as the native calls take it: an int in [0, 255], refused here before any native call"""
    if isinstance(repeat, (bool, np.bool_)) or not isinstance(repeat, (int, np.integer)) or not 0 <= int(repeat) <= 255:
        raise ValueError(f"repeat must be an int in [0, 255] (skipped frames per decision), got {repeat!r}")
    return int(repeat)


def _count(value, name, low, high=None):
    """an int argument in [low, high] as the native calls take it, refused here before any native call"""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or int(value) < low or (high is not None and int(value) > high):
        raise ValueError(f"{name} must be an int {'>= %d' % low if high is None else 'in [%d, %d]' % (low, high)}, got {value!r}")
    return int(value)


def _logp_buffer(x, shape, name, device=None):
    """a device float32 tensor of exactly `shape` for log-probabilities, refused here before any native call"""
    if not hasattr(x, "data_ptr") or not hasattr(x, "dtype") or not hasattr(x, "shape"):
        raise ValueError(f"{name} must be a device float32 tensor of shape {tuple(shape)}, got {type(x).__name__}")
    if str(x.dtype) != "torch.float32":
        raise ValueError(f"{name} must be float32, got {x.dtype}")
    if tuple(int(v) for v in x.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(x.shape)}")
    if not getattr(x, "is_cuda", False):
        raise ValueError(f"{name} must be on the handle's device, got a host tensor")
    index = getattr(getattr(x, "device", None), "index", None)
    if device is not None and index is not None and int(index) != int(device):
        raise ValueError(f"{name} is on device {index}, the handle on {device}")
    if not x.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return x


class BatchStep:
    """What `Step[]` (IVecEnv.cs:15) becomes at 2^20 lanes: three arrays.  Indexing / iterating yields the
    reference's per-env Step records (Step.cs:7-20), materialised lazily."""
    __slots__ = ("Observation", "Reward", "Done", "Information", "Truncated")

    def __init__(self, observation, reward, done, information=None, truncated=None):
        self.Observation, self.Reward, self.Done, self.Information = observation, reward, done, information
        self.Truncated = truncated          # bool [N]: the episode ended by the max_episode_steps extension (done byte, bit 1)

    def __len__(self):
        return self.Reward.shape[0]

    def __getitem__(self, i):
        info = self.Information
        if self.Truncated is not None and self.Truncated[i]:
            info = {"TimeLimit.truncated": True}                  # upstream gym's TimeLimit convention (the reference has none)
        return Step(self.Observation[i], float(self.Reward[i]), bool(self.Done[i]), info)

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]

    def ToSteps(self):
        return list(self)


class PendingStep:
    """Task<Step[]> of VecEnv.StepAsync (VecEnv.cs:63-65): Result() blocks like Task.Result."""

    def __init__(self, env):
        self._env, self._result = env, None

    def Result(self):
        if self._result is None:
            self._result = self._env.StepWait()
        return self._result


class VectorEnv:
    def __init__(self, env="CartPole-v1", num_envs=1, device=0, seed=0, auto_reset=False,
                 validate_actions=False, done_list=False, episode_stats=False, final_obs=False,
                 lane_offset=0, stream=None, ext_obs=None, ext_obs_stride=0, max_episode_steps=0,
                 double_buffer=False, ext_obs_alt=None, dtype=np.float32, compact_records_only=False, launch_policy=None, resident=False):
        """dtype=np.float64 (CartPole only) selects GYMNET_FLAG_F64: the reference's own float64 arithmetic, float64 state and
        float64 observations (what CartPoleEnv.Step actually returns, CartPoleEnv.cs:166,185); the default float32 is the
        engine's structure-of-arrays hot path.  resident=True (num_envs <= 64): GYMNET_FLAG_RESIDENT — Step / Reset / ResetWhere(None)
        are served by a resident single-wave kernel through a mailbox in pinned host memory (no launch, no synchronize per step).  launch_policy: dict for SetLaunchPolicy (probes / tests that pin a kernel form)."""
        env_id = capi.ENV_IDS[env] if isinstance(env, str) else int(env)
        self._lib = capi.load_library()
        self._info = capi.env_describe(env_id)
        self._dtype = np.dtype(dtype)
        if self._dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("dtype must be float32 or float64")
        flags = ((capi.FLAG_AUTORESET if auto_reset else 0) | (capi.FLAG_VALIDATE_ACTIONS if validate_actions else 0)
                 | (capi.FLAG_DONE_LIST if done_list else 0) | (capi.FLAG_EPISODE_STATS if episode_stats else 0)
                 | (capi.FLAG_FINAL_OBS if final_obs else 0) | (capi.FLAG_DOUBLE_BUFFER if double_buffer else 0)
                 | (capi.FLAG_F64 if self._dtype == np.float64 else 0)
                 | (capi.FLAG_COMPACT_RECORDS_ONLY if compact_records_only else 0)
                 | (capi.FLAG_RESIDENT if resident else 0))
        cfg = capi.Config(struct_size=C.sizeof(capi.Config), env_id=env_id, num_envs=int(num_envs),
                          lane_offset=int(lane_offset), device=int(device), flags=flags,
                          seed=int(seed) & 0xFFFFFFFFFFFFFFFF, stream=_ptr(stream), d_ext_obs=_ptr(ext_obs),
                          ext_obs_stride=int(ext_obs_stride), max_episode_steps=int(max_episode_steps), reserved=0,
                          d_ext_obs_alt=_ptr(ext_obs_alt))
        self._h = C.c_void_p()
        self._owns_handle = True
        self._bookkeeping = bool(episode_stats or max_episode_steps)
        self._final_obs = bool(final_obs)
        self.Resident = bool(resident)
        self.Device = int(device)
        capi.check(self._lib.gymnet_vecenv_create(C.byref(cfg), C.byref(self._h)))
        self._describe(env_id, num_envs, auto_reset)
        if launch_policy:
            self.SetLaunchPolicy(**launch_policy)

    @classmethod
    def _borrow(cls, handle, env_id, num_envs, auto_reset, dtype=np.float32):
        """A VectorEnv view over a handle somebody else owns (a member of a GroupVectorEnv): Close() does not destroy it."""
        self = cls.__new__(cls)
        self._lib = capi.load_library()
        self._info = capi.env_describe(env_id)
        self._h = handle
        self._owns_handle = False
        self._bookkeeping = True            # a group member: flags unknown here (DoneRecords() asks for everything it may have)
        self._final_obs = False
        self.Resident = False
        self.Device = None                  # not known here: PixelStack needs an `out` tensor
        self._dtype = np.dtype(dtype)
        self._describe(env_id, num_envs, auto_reset)
        return self

    def _describe(self, env_id, num_envs, auto_reset):
        i = self._info
        self.EnvId = env_id
        self.Name = i.name.decode()
        self.NumberOfEnvironments = int(num_envs)                                   # VecEnv.cs:14,24
        self.StateDim, self.ObsDim = int(i.state_dim), int(i.obs_dim)
        self.AutoReset = bool(auto_reset)
        # spaces exactly as the env ctor builds them (CartPoleEnv.cs:46-48)
        if i.action_is_box:
            self.ActionSpace = Box(np.array([i.action_low], np.float32), np.array([i.action_high], np.float32), dtype=np.float32)
            self._adtype = np.float32
        else:
            self.ActionSpace = Discrete(int(i.action_n))
            self._adtype = np.int32
        # the DECLARED dtype stays float32 (CartPoleEnv.cs:48) even when the arrays returned are float64, exactly as in the reference
        self.ObservationSpace = Box(np.array(i.obs_low[:self.ObsDim], np.float32), np.array(i.obs_high[:self.ObsDim], np.float32), dtype=np.float32)
        self.Dtype = self._dtype            # dtype of the observation / state arrays this handle hands out
        self.Metadata = {"render.modes": ["human", "rgb_array"], "video.frames_per_second": 50}   # CartPoleEnv.cs:51
        self.RewardRange = (float(i.reward_low), float(i.reward_high))
        self.Environments = []          # VecEnv.cs:17 — deliberately empty, see module docstring
        self.AlgorithmicBytesPerStep = int(i.algorithmic_bytes_per_step)
        self.TrafficBytesPerStep = int(i.traffic_bytes_per_step)      # < algorithmic where a state row is stored once, in the observation

    # ---- lifecycle ------------------------------------------------------------------------------
    def Close(self):                                                                 # VecEnvWrapper.cs:26-30
        if getattr(self, "_h", None) is not None and self._h:
            self._pinned = None                     # views over memory the handle owns
            if self._owns_handle:
                self._lib.gymnet_vecenv_destroy(self._h)
            self._h = C.c_void_p()

    Dispose = Close                                                                  # Env.cs:38-40

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.Close()

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass

    def Seed(self, seed):                                                            # VecEnv.cs:44-53
        if isinstance(seed, (int, np.integer)):
            capi.check(self._lib.gymnet_vecenv_seed(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF))
        else:
            s = np.ascontiguousarray(np.asarray(seed, dtype=np.int64).astype(np.uint64))
            capi.check(self._lib.gymnet_vecenv_seed_lanes(self._h, _host(s), s.shape[0]))

    # ---- host-boundary path ---------------------------------------------------------------------
    def _outs(self):
        n = self.NumberOfEnvironments
        return (np.empty((n, self.ObsDim), self._dtype), np.empty(n, np.float32), np.empty(n, np.uint8))

    def Reset(self):                                                                 # VecEnvWrapper.cs:18-20
        obs = np.empty((self.NumberOfEnvironments, self.ObsDim), self._dtype)
        capi.check(self._lib.gymnet_vecenv_reset(self._h, _host(obs)))
        return obs

    def ResetWhere(self, mask=None):
        """Batched `if (done) Reset()` (README.md:36-40). mask None = lanes whose last Done flag is set."""
        obs = np.empty((self.NumberOfEnvironments, self.ObsDim), self._dtype)
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
        if m is not None and m.shape[0] != self.NumberOfEnvironments:
            raise ValueError("mask length must equal NumberOfEnvironments")
        capi.check(self._lib.gymnet_vecenv_reset_where(self._h, None if m is None else _host(m), _host(obs)))
        return obs

    def _actions(self, action):
        a = np.ascontiguousarray(np.asarray(action).reshape(-1).astype(self._adtype, copy=False))
        if a.shape[0] != self.NumberOfEnvironments:
            raise ValueError("Number of actions passed should be equals to number of environments")
        return a

    def Step(self, action):
        """IVecEnv.Step(int action) (IVecEnv.cs:15, VecEnvWrapper.cs:22-24) broadcasts ONE scalar action;
        an array-like gives one action per lane (extension)."""
        obs, rew, done = self._outs()
        if isinstance(action, enum.Enum):                                            # Env<TAction>.Step(TAction), Env.cs:43-53
            action = int(action.value)
        if isinstance(action, (int, np.integer)) and not isinstance(action, (bool, np.bool_)):
            capi.check(self._lib.gymnet_vecenv_step_broadcast(self._h, int(action), _host(obs), _host(rew), _host(done)))
        else:
            a = self._actions(action)
            capi.check(self._lib.gymnet_vecenv_step(self._h, _host(a), _host(obs), _host(rew), _host(done)))
        return BatchStep(obs, rew, done.astype(bool), None, truncated=(done & 2) != 0)

    def StepRepeat(self, action, repeat):
        """Frame skip at the host boundary (gymnet_vecenv_step_repeat): one action per lane, held for repeat + 1 env steps in one launch.
        The BatchStep carries the decision's observation (post-reset where a lane finished), its summed reward and its done byte; a
        lane that finishes inside the decision stops there (see StepRepeatDevice).  repeat = 0 is Step(action) with an array."""
        repeat = _repeat(repeat)
        obs, rew, done = self._outs()
        a = self._actions(action)
        capi.check(self._lib.gymnet_vecenv_step_repeat(self._h, _host(a), repeat, _host(obs), _host(rew), _host(done)))
        return BatchStep(obs, rew, done.astype(bool), None, truncated=(done & 2) != 0)

    def HostBuffers(self):
        """(actions, obs, reward, done): numpy views over the library's page-locked, device-mapped host buffers
        (gymnet_vecenv_host_buffers).  Passing them to StepInto / ResetInto runs the host boundary without staging copies."""
        if getattr(self, "_pinned", None) is None:
            a, o, r, d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
            capi.check(self._lib.gymnet_vecenv_host_buffers(self._h, C.byref(a), C.byref(o), C.byref(r), C.byref(d)))
            n, D = self.NumberOfEnvironments, self.ObsDim

            def view(ptr, ctype, count, dtype, shape):
                return np.frombuffer((ctype * count).from_address(ptr.value), dtype=dtype).reshape(shape)
            self._pinned = (view(a, C.c_int32, n, self._adtype, (n,)),
                            view(o, C.c_double if self._dtype == np.float64 else C.c_float, n * D, self._dtype, (n, D)),
                            view(r, C.c_float, n, np.float32, (n,)), view(d, C.c_uint8, n, np.uint8, (n,)))
        return self._pinned

    def StepInto(self, actions, obs_out, reward_out, done_out):
        """gymnet_vecenv_step with CALLER-OWNED buffers (what a C# host with long-lived NDArrays does): actions [N] of the
        action dtype, obs_out float32 [N, D], reward_out float32 [N], done_out uint8 [N]; nothing is allocated."""
        n = self.NumberOfEnvironments
        if (actions.dtype != self._adtype or obs_out.dtype != self._dtype or reward_out.dtype != np.float32 or done_out.dtype != np.uint8
                or actions.shape != (n,) or obs_out.shape != (n, self.ObsDim) or reward_out.shape != (n,) or done_out.shape != (n,)
                or not (actions.flags.c_contiguous and obs_out.flags.c_contiguous and reward_out.flags.c_contiguous and done_out.flags.c_contiguous)):
            raise ValueError("StepInto needs C-contiguous buffers of the exact dtypes and shapes")
        capi.check(self._lib.gymnet_vecenv_step(self._h, _host(actions), _host(obs_out), _host(reward_out), _host(done_out)))

    def ResetInto(self, obs_out):
        if obs_out.dtype != self._dtype or obs_out.shape != (self.NumberOfEnvironments, self.ObsDim) or not obs_out.flags.c_contiguous:
            raise ValueError("ResetInto needs a C-contiguous [N, D] buffer of the handle's dtype")
        capi.check(self._lib.gymnet_vecenv_reset(self._h, _host(obs_out)))

    def StepAsync(self, action):                                                     # VecEnv.cs:63-65
        if isinstance(action, enum.Enum):
            action = int(action.value)
        if isinstance(action, (int, np.integer)):
            action = np.full(self.NumberOfEnvironments, action, dtype=self._adtype)
        a = self._actions(action)
        capi.check(self._lib.gymnet_vecenv_step_async(self._h, _host(a)))
        return PendingStep(self)

    def StepWait(self):
        obs, rew, done = self._outs()
        capi.check(self._lib.gymnet_vecenv_step_wait(self._h, _host(obs), _host(rew), _host(done)))
        return BatchStep(obs, rew, done.astype(bool), None, truncated=(done & 2) != 0)

    def Read(self):
        obs, rew, done = self._outs()
        capi.check(self._lib.gymnet_vecenv_read(self._h, _host(obs), _host(rew), _host(done)))
        return BatchStep(obs, rew, done.astype(bool), None, truncated=(done & 2) != 0)

    def SampleActions(self, seed=0, tick=0):
        """ActionSpace.Sample() for every lane, on the device (TrainingPlaySession.cs:46-49 batched)."""
        a = np.empty(self.NumberOfEnvironments, self._adtype)
        capi.check(self._lib.gymnet_vecenv_sample_actions(self._h, _host(a), int(seed), int(tick)))
        return a

    # ---- device-resident path (device pointers: ints, ctypes pointers or torch tensors) -------------
    # The stream contract of every *Device method, of this class and of PixelFrameStack, EpisodeMemory and Actor (include/gymnet_amd.h,
    # "device-resident path"): all of the call's work is queued on the handle's stream (stream= at construction, or the library's own), in
    # call order, and the call returns without waiting for it.  With validate_actions=True StepDevice, StepRepeatDevice and RolloutDevice
    # block (one readback answers Discrete.Contains before any state changes); a call may block the first time it needs storage the handle
    # allocates on demand (a fused rollout's episode records).  None of them may be captured by the caller into a graph of its own
    # (torch.cuda.graph): the handle keeps host-side counters a replay would not advance.  The handle-less exports behind AdvantagesDevice
    # and RolloutInputsDevice (gymnet_gae_device, gymnet_rollout_inputs_device), the gymnet_sample_*_device samplers and
    # gymnet_push_obs_device keep nothing and are capturable when called through the C ABI with the capturing stream.
    def ResetDevice(self):
        capi.check(self._lib.gymnet_vecenv_reset_device(self._h))

    def ResetWhereDevice(self, d_mask=None):
        capi.check(self._lib.gymnet_vecenv_reset_where_device(self._h, _ptr(d_mask)))

    def StepDevice(self, d_actions):
        capi.check(self._lib.gymnet_vecenv_step_device(self._h, _ptr(d_actions)))

    def StepRepeatDevice(self, d_actions, repeat):
        """One DECISION (gymnet_vecenv_step_repeat_device): d_actions held for R = repeat + 1 env steps inside one launch — the
        reference's SkippedFrames (BasePlaySession.cs:37-56).  A lane whose done byte comes out non-zero at a sub-step keeps that byte,
        is reset there on an auto_reset handle, and idles for the rest of the decision; the reward is the sum of the sub-step rewards
        taken; the tick advances by R.  repeat = 0 is StepDevice."""
        repeat = _repeat(repeat)
        capi.check(self._lib.gymnet_vecenv_step_repeat_device(self._h, _ptr(d_actions), repeat))

    def RolloutDevice(self, d_actions, steps, action_stride, ring):
        capi.check(self._lib.gymnet_vecenv_rollout_device(self._h, _ptr(d_actions), int(steps), int(action_stride), int(ring)))

    def RolloutFusedDevice(self, d_actions, steps, action_stride=0, ring=1, rec_obs=None, rec_reward=None, rec_done=None, actions="ring",
                           action_seed=0, action_tick0=0, epsilon=0.0, rec_actions=None, episodes=None, repeat=0, rec_logp=None, rec_value=None, rec_logd=None,
                           rec_boot=None):
        """`steps` vector steps in ONE kernel launch (state stays in registers); optional device-side rollout
        buffers rec_obs [T][D][N] (of the handle's dtype: float64 for a float64 handle), rec_reward [T][N], rec_done [T][N]
        (ReplayMemory.cs:25-67, batched).  gymnet_vecenv_rollout_fused_ex_device:
          actions   "ring" (d_actions[t % ring]), "sample" (ActionSpace.Sample() drawn in the kernel: the values SampleActionsDevice
                    (seed=action_seed, tick=action_tick0 + t) would write; d_actions may be None) or "epsilon_greedy" (ComposeActionsDevice
                    over d_actions as the policy's actions, TrainingPlaySession.cs:46-52) or "actor" (the handle's Actor chooses
                    step t's action as Act(epsilon, action_seed, action_tick0 + t) would, and keeps its history current; d_actions
                    may be None)
          rec_actions  [T][N] device buffer for the actions taken (int32; float32 on a Box-action env)
          episodes  dict(step=, lane=, ret=, length=, capacity=, count=): device arrays for the compact records of the episodes
                    that end during the rollout (any array may be omitted; count: uint32[2] = records written, episodes ended);
                    no_overflow=True selects the 8 % faster kernel variant that may drop records of very unevenly finishing lanes
                    below `capacity` (GYMNET_RECORDS_NO_OVERFLOW; count[1] > count[0] says so);
                    needs a bookkeeping handle (BasePlaySession.cs:58-69).
          repeat    frame skip (gymnet_vecenv_rollout_repeat_device): `steps` counts DECISIONS, each action is held for repeat + 1 env
                    steps, the rec_* buffers and the records' step index are per decision ("actor" needs repeat = 0).
          rec_logp  device float32 [T, N] for the log-probability of every action taken, as Actor.Act(logp=) writes it at that step
                    (gymnet_vecenv_rollout_fused_logp_device): needs actions="actor" on a Discrete actor.
          rec_value device float32 [T, N] or [T + 1, N] for the critic's value of the input every action was chosen from, as
                    Actor.Value() would write it before that step (gymnet_vecenv_rollout_fused_value_device): needs actions="actor" on a
                    Discrete actor with a critic (Actor.SetCritic).  With T + 1 rows, row T takes Actor.Value() after the rollout — the
                    last value — and AdvantagesDevice(rec_reward, rec_done, rec_value, ...) takes the tensor as it stands.  On a Box actor
                    rec_value is accepted together with rec_logd, in either shape.
          rec_logd  device float32 [T, N] for the log-density of every action taken, as Actor.Act(logd=) writes it at that step
                    (gymnet_vecenv_rollout_fused_box_logd_device): needs actions="actor" on a Box actor whose policy has sigma > 0, and
                    repeat = 0.
          rec_boot  device float32 [T, N] for V(terminal observation) on time-limit rows, as Actor.Boot() writes it after that step
                    (+0.0 on every other row): what AdvantagesDevice takes as boot= (gymnet_vecenv_rollout_fused_value_boot_device,
                    _box_boot_device).  Needs rec_value (on a Box actor rec_logd too), actions="actor", repeat = 0 and a handle with
                    max_episode_steps > 0; final_obs is not needed."""
        repeat = _repeat(repeat)
        value_rows = None
        if rec_boot is not None:
            if actions != "actor":
                raise ValueError(f"rec_boot records the critic's value of terminal observations where the actor chooses: it needs actions=\"actor\", got {actions!r}")
            if rec_value is None:
                raise ValueError("rec_boot needs rec_value (V(terminal observation) is recorded beside the values)")
            if repeat:
                raise ValueError("rec_boot: the fused actor rollout has no frame skip (repeat must be 0)")
            _logp_buffer(rec_boot, (_count(steps, "steps", 0), self.NumberOfEnvironments), "rec_boot", self.Device)
        box_logd = rec_logd is not None
        if box_logd:
            actor = getattr(self, "_actor", None)
            if actions != "actor":
                raise ValueError(f"rec_logd records the actor's log-densities: it needs actions=\"actor\", got {actions!r}")
            if actor is None:
                raise ValueError("rec_logd needs an actor (VectorEnv.Actor)")
            if not actor.IsBox:
                raise ValueError("rec_logd belongs to a Box actor; this handle's actor chooses Discrete actions (rec_logp)")
            if rec_logp is not None:
                raise ValueError("rec_logp belongs to a Discrete actor; this handle's actor chooses Box actions (rec_logd)")
            if repeat:
                raise ValueError("rec_logd: the fused actor rollout has no frame skip (repeat must be 0)")
            T = _count(steps, "steps", 0)
            _logp_buffer(rec_logd, (T, self.NumberOfEnvironments), "rec_logd", self.Device)
            if rec_value is not None:
                if getattr(actor, "CriticWidths", None) is None:
                    raise ValueError("rec_value needs a critic (Actor.SetCritic)")
                value_rows = T + 1 if tuple(getattr(rec_value, "shape", ()))[:1] == (T + 1,) else T
                _logp_buffer(rec_value, (value_rows, self.NumberOfEnvironments), "rec_value", self.Device)
        if rec_value is not None and not box_logd:
            actor = getattr(self, "_actor", None)
            if actions != "actor":
                raise ValueError(f"rec_value records the critic's values where the actor chooses: it needs actions=\"actor\", got {actions!r}")
            if actor is None:
                raise ValueError("rec_value needs an actor (VectorEnv.Actor)")
            if actor.IsBox:
                raise ValueError("rec_value alone belongs to a Discrete actor's fused rollout; this handle's actor chooses Box actions: pass "
                                 "rec_logd with it (Actor.Value serves a single step)")
            if getattr(actor, "CriticWidths", None) is None:
                raise ValueError("rec_value needs a critic (Actor.SetCritic)")
            if repeat:
                raise ValueError("rec_value: the fused actor rollout has no frame skip (repeat must be 0)")
            T = _count(steps, "steps", 0)
            value_rows = T + 1 if tuple(getattr(rec_value, "shape", ()))[:1] == (T + 1,) else T
            _logp_buffer(rec_value, (value_rows, self.NumberOfEnvironments), "rec_value", self.Device)
        if rec_logp is not None and not box_logd:
            actor = getattr(self, "_actor", None)
            if actions != "actor":
                raise ValueError(f"rec_logp records the actor's log-probabilities: it needs actions=\"actor\", got {actions!r}")
            if actor is None:
                raise ValueError("rec_logp needs an actor (VectorEnv.Actor)")
            if actor.IsBox:
                raise ValueError("rec_logp belongs to a Discrete actor; this handle's actor chooses Box actions")
            if repeat:
                raise ValueError("rec_logp: the fused actor rollout has no frame skip (repeat must be 0)")
            _logp_buffer(rec_logp, (_count(steps, "steps", 0), self.NumberOfEnvironments), "rec_logp", self.Device)
        src = {"ring": capi.ACTIONS_RING, "sample": capi.ACTIONS_SAMPLE, "epsilon_greedy": capi.ACTIONS_EPSILON_GREEDY,
               "actor": capi.ACTIONS_ACTOR}[actions]
        ep = episodes or {}
        unknown = set(ep) - {"step", "lane", "ret", "length", "capacity", "count", "no_overflow"}
        if unknown:
            raise TypeError(f"unknown episode record field(s): {sorted(unknown)}")
        spec = capi.RolloutSpec(struct_size=C.sizeof(capi.RolloutSpec), action_source=src, d_actions=_ptr(d_actions), steps=int(steps),
                                action_stride=int(action_stride), ring=int(ring), action_seed=int(action_seed) & 0xFFFFFFFFFFFFFFFF,
                                action_tick0=int(action_tick0), epsilon=float(epsilon), record_flags=capi.RECORDS_NO_OVERFLOW if ep.get("no_overflow") else 0,
                                d_rec_obs=_ptr(rec_obs), d_rec_reward=_ptr(rec_reward), d_rec_done=_ptr(rec_done), d_rec_actions=_ptr(rec_actions),
                                d_ep_step=_ptr(ep.get("step")), d_ep_lane=_ptr(ep.get("lane")), d_ep_return=_ptr(ep.get("ret")),
                                d_ep_length=_ptr(ep.get("length")), ep_capacity=int(ep.get("capacity", 0)), d_ep_count=_ptr(ep.get("count")))
        if repeat:
            capi.check(self._lib.gymnet_vecenv_rollout_repeat_device(self._h, C.byref(spec), repeat))
        elif box_logd:
            if rec_boot is not None:
                capi.check(self._lib.gymnet_vecenv_rollout_fused_box_boot_device(self._h, C.byref(spec), _ptr(rec_logd), _ptr(rec_value), _ptr(rec_boot)))
            else:
                capi.check(self._lib.gymnet_vecenv_rollout_fused_box_logd_device(self._h, C.byref(spec), _ptr(rec_logd), _ptr(rec_value)))
            if value_rows == int(steps) + 1:                  # row T: the value of the history the rollout leaves
                last = C.c_void_p(rec_value.data_ptr() + 4 * int(steps) * self.NumberOfEnvironments)
                capi.check(self._lib.gymnet_vecenv_actor_value_device(self._h, last))
        elif rec_value is not None:
            if rec_boot is not None:
                capi.check(self._lib.gymnet_vecenv_rollout_fused_value_boot_device(self._h, C.byref(spec), _ptr(rec_logp), _ptr(rec_value), _ptr(rec_boot)))
            else:
                capi.check(self._lib.gymnet_vecenv_rollout_fused_value_device(self._h, C.byref(spec), _ptr(rec_logp), _ptr(rec_value)))
            if value_rows == int(steps) + 1:                  # row T: the value of the history the rollout leaves
                last = C.c_void_p(rec_value.data_ptr() + 4 * int(steps) * self.NumberOfEnvironments)
                capi.check(self._lib.gymnet_vecenv_actor_value_device(self._h, last))
        elif rec_logp is not None:
            capi.check(self._lib.gymnet_vecenv_rollout_fused_logp_device(self._h, C.byref(spec), _ptr(rec_logp)))
        else:
            capi.check(self._lib.gymnet_vecenv_rollout_fused_ex_device(self._h, C.byref(spec)))

    def AdvantagesDevice(self, reward, done, values, advantage, returns, gamma=0.99, lam=0.95, last_value=None, boot=None):
        """GAE(gamma, lam) advantages and advantage + value over the rows a rollout recorded, in one kernel launch on the handle's
        device and stream (gymnet_gae_device: the recurrence is written out there), so it is ordered after the rollout with no
        synchronise.  reward float32 [T, n] and done uint8 [T, n] are RolloutFusedDevice's rec_reward / rec_done (n = the handle's lanes).
          values     None (every value is 0: with lam = 1 the advantage is the discounted reward-to-go), float32 [T, n] with last_value
                     float32 [n] (None: 0), or float32 [T + 1, n] whose row T is the last value (last_value must then be None).
                     values[t] is the value of the observation step t's action was chosen from: values[0] = V(observation before the
                     rollout), values[t] = V(rec_obs[t - 1]), last value = V(rec_obs[T - 1])
          boot       float32 [T, n]: V(terminal observation) where a time limit truncated the lane (done bit 1); None: a truncation counts
                     as a termination
          advantage, returns   caller-allocated float32 [T, n]; either may be None, not both.  advantage may be the reward tensor while
                     returns is values' first T rows, or the other way round: each element is read before it is written.
        Every argument is checked here, before any native call."""
        dev = self.Device
        reward = _logp_buffer(reward, getattr(reward, "shape", ()), "reward", dev)
        if len(reward.shape) != 2 or int(reward.shape[1]) != self.NumberOfEnvironments:
            raise ValueError(f"reward must have shape (T, {self.NumberOfEnvironments}), got {tuple(reward.shape)}")
        T, n = int(reward.shape[0]), self.NumberOfEnvironments
        if not hasattr(done, "data_ptr") or str(getattr(done, "dtype", None)) != "torch.uint8":
            raise ValueError(f"done must be a device uint8 tensor of shape ({T}, {n}), got {getattr(done, 'dtype', type(done).__name__)}")
        if tuple(int(v) for v in done.shape) != (T, n) or not getattr(done, "is_cuda", False) or not done.is_contiguous():
            raise ValueError(f"done must be a contiguous device tensor of shape ({T}, {n}), got {tuple(done.shape)}")
        index = getattr(getattr(done, "device", None), "index", None)
        if dev is not None and index is not None and int(index) != int(dev):
            raise ValueError(f"done is on device {index}, the handle on {dev}")
        v_ptr = lv_ptr = None
        if values is not None:
            rows = int(values.shape[0]) if len(getattr(values, "shape", ())) == 2 else -1
            if rows == T + 1:
                if last_value is not None:
                    raise ValueError("values has T + 1 rows (row T is the last value): last_value must be None")
                _logp_buffer(values, (T + 1, n), "values", dev)
                lv_ptr = C.c_void_p(values.data_ptr() + 4 * T * n)
            else:
                _logp_buffer(values, (T, n), "values", dev)
            v_ptr = _ptr(values)
        if last_value is not None:
            lv_ptr = _ptr(_logp_buffer(last_value, (n,), "last_value", dev))
        if boot is not None:
            _logp_buffer(boot, (T, n), "boot", dev)
        if advantage is None and returns is None:
            raise ValueError("advantage and returns are both None")
        if advantage is not None:
            _logp_buffer(advantage, (T, n), "advantage", dev)
        if returns is not None:
            if values is not None and returns is values and int(values.shape[0]) == T + 1:
                pass                                          # in place over the first T rows of a [T + 1, n] values tensor
            else:
                _logp_buffer(returns, (T, n), "returns", dev)
        for name, g in (("gamma", gamma), ("lam", lam)):
            if isinstance(g, (bool, np.bool_)) or not isinstance(g, (int, float, np.integer, np.floating)) or not 0.0 <= float(g) <= 1.0:
                raise ValueError(f"{name} must be a number in [0, 1], got {g!r}")
        if dev is None:
            dev = getattr(getattr(reward, "device", None), "index", None)
            if dev is None:
                raise ValueError("the handle's device is not known and reward does not name one")
        stream = self.DeviceView().stream
        capi.check(self._lib.gymnet_gae_device(int(dev), C.c_void_p(stream), T, n, n, _ptr(reward), _ptr(done), v_ptr, lv_ptr, _ptr(boot),
                                               float(gamma), float(lam), _ptr(advantage), _ptr(returns)))

    def RolloutInputsDevice(self, rec_obs, rec_done, history0, history, rows=None, out=None, history_out=None):
        """The network inputs a recorded rollout's actions were chosen from, on the handle's device and stream (gymnet_rollout_inputs_device:
        the rule is written out there), so it is ordered after the rollout with no synchronise.  For step t of a lane: the lane's last
        `history` observations before the step, oldest first, clamped to the episode's first — what Actor.Act read.
          rec_obs    RolloutFusedDevice's rec_obs, [T, obs_dim, n] float32, or float64 (a float64 handle's; each value is rounded to float32)
          rec_done   its rec_done, uint8 [T, n]
          history0   float32 [history, obs_dim, n]: Actor.HistoryDevice() taken before the rollout (or a previous call's history_out)
          rows       None: every row, the result is float32 [T, n, history * obs_dim]; or a device int64 tensor [m] of flat row indices
                     t * n + lane (a PPO minibatch; duplicates allowed): the result is [m, history * obs_dim].  An index outside
                     [0, T * n) gives a row of NaN.
          out        the result's tensor, caller-allocated (contiguous, of exactly that shape); None: a new one.  Returned.
          history_out  optional float32 [history, obs_dim, n]: the history after the last step, the next call's history0
        Every argument is checked here, before any native call."""
        dev, n = self.Device, self.NumberOfEnvironments
        S = _count(history, "history", 1, 64)
        if not hasattr(rec_obs, "data_ptr") or str(getattr(rec_obs, "dtype", None)) not in ("torch.float32", "torch.float64"):
            raise ValueError(f"rec_obs must be a device float32 or float64 tensor [T, obs_dim, {n}], got {getattr(rec_obs, 'dtype', type(rec_obs).__name__)}")
        f64 = str(rec_obs.dtype) == "torch.float64"
        shape = tuple(int(v) for v in rec_obs.shape)
        if len(shape) != 3 or shape[2] != n or shape[1] < 1:
            raise ValueError(f"rec_obs must have shape (T, obs_dim, {n}), got {shape}")
        T, O = shape[0], shape[1]
        if S * O > 64:
            raise ValueError(f"history * obs_dim = {S * O} is beyond 64, the widest input an actor can have")

        def device_tensor(x, want, dtype, name):
            if not hasattr(x, "data_ptr") or str(getattr(x, "dtype", None)) != dtype:
                raise ValueError(f"{name} must be a device {dtype[6:]} tensor of shape {want}, got {getattr(x, 'dtype', type(x).__name__)}")
            if want is not None and tuple(int(v) for v in x.shape) != tuple(want):
                raise ValueError(f"{name} must have shape {tuple(want)}, got {tuple(x.shape)}")
            if not getattr(x, "is_cuda", False) or not x.is_contiguous():
                raise ValueError(f"{name} must be a contiguous tensor on the handle's device")
            index = getattr(getattr(x, "device", None), "index", None)
            if dev is not None and index is not None and int(index) != int(dev):
                raise ValueError(f"{name} is on device {index}, the handle on {dev}")
            return x
        device_tensor(rec_obs, shape, str(rec_obs.dtype), "rec_obs")
        device_tensor(rec_done, (T, n), "torch.uint8", "rec_done")
        device_tensor(history0, (S, O, n), "torch.float32", "history0")
        if history_out is not None:
            device_tensor(history_out, (S, O, n), "torch.float32", "history_out")
        m = 0
        if rows is not None:
            device_tensor(rows, None, "torch.int64", "rows")
            if len(rows.shape) != 1:
                raise ValueError(f"rows must be one-dimensional, got shape {tuple(rows.shape)}")
            m = int(rows.shape[0])
        want = (T, n, S * O) if rows is None else (m, S * O)
        if dev is None:
            dev = getattr(getattr(rec_obs, "device", None), "index", None)
            if dev is None:
                raise ValueError("the handle's device is not known and rec_obs does not name one")
        if out is None:
            import torch
            out = torch.empty(want, dtype=torch.float32, device=f"cuda:{int(dev)}")
        else:
            device_tensor(out, want, "torch.float32", "out")
        if rows is not None and m == 0:
            return out                                        # the gathered form with no row is a no-op (an empty tensor has no pointer)
        stream = self.DeviceView().stream
        capi.check(self._lib.gymnet_rollout_inputs_device(int(dev), C.c_void_p(stream), T, n, n, O, S, 1 if f64 else 0, _ptr(rec_obs), _ptr(rec_done),
                                                          _ptr(history0), n, _ptr(rows), m, _ptr(out), S * O, _ptr(history_out), n))
        return out

    def SampleActionsDevice(self, d_actions, seed=0, tick=0):
        capi.check(self._lib.gymnet_vecenv_sample_actions_device(self._h, _ptr(d_actions), int(seed), int(tick)))

    def SampleActionsMaskedDevice(self, d_actions, d_mask, per_lane=True, seed=0, tick=0):
        """ActionSpace.Sample(mask) for every lane (Discrete.cs:18-26): d_mask uint8 [N][n] (per_lane) or one shared row [n]."""
        stride = self.ActionSpace.N if per_lane else 0
        capi.check(self._lib.gymnet_vecenv_sample_actions_masked_device(self._h, _ptr(d_actions), _ptr(d_mask), int(stride),
                                                                        int(seed), int(tick)))

    def ComposeActionsDevice(self, d_policy_actions, epsilon, d_actions_out, seed=0, tick=0):
        """Batched epsilon-greedy ComposeAction (TrainingPlaySession.cs:46-52): with probability epsilon the lane's
        action is ActionSpace.Sample(), otherwise the policy's."""
        capi.check(self._lib.gymnet_vecenv_compose_actions_device(self._h, _ptr(d_policy_actions), float(epsilon),
                                                                  _ptr(d_actions_out), int(seed), int(tick)))

    # ---- CartPole frames (CartPoleEnv.Render, CartPoleEnv.cs:69-135; contract: gymnet_vecenv_render_device) -----------------
    _FORMATS = {"rgb": capi.PIXELS_RGB8, "gray": capi.PIXELS_GRAY8, capi.PIXELS_RGB8: capi.PIXELS_RGB8, capi.PIXELS_GRAY8: capi.PIXELS_GRAY8}
    _CANVAS = (0, 0, capi.RENDER_WIDTH, capi.RENDER_HEIGHT)

    def _render_args(self, format, first_lane, count, crop, size, lane_stride):
        fmt = self._FORMATS.get(format)
        if fmt is None:
            raise ValueError(f"unknown pixel format {format!r} (\"rgb\" or \"gray\")")
        cx, cy, cw, ch = (int(v) for v in crop)
        w, h = (cw, ch) if size is None else (int(size[0]), int(size[1]))
        count = self.NumberOfEnvironments - int(first_lane) if count is None else int(count)
        frame = w * h * (3 if fmt == capi.PIXELS_RGB8 else 1)
        return (fmt, int(first_lane), count, cx, cy, cw, ch, w, h, frame if lane_stride is None else int(lane_stride))

    def RenderDevice(self, d_out, format="gray", first_lane=0, count=None, crop=_CANVAS, size=None, lane_stride=None):
        """Frames of lanes [first_lane, first_lane + count) into device memory (a torch tensor or an int pointer), ordered on the
        handle's stream: format "rgb" (out_h x out_w x 3 bytes) or "gray" (out_h x out_w), crop = (x, y, w, h) of the 600 x 400 canvas,
        size = (out_w, out_h) (default: the crop's size), lane k's frame at d_out + (k - first_lane) * lane_stride bytes (default:
        frames back to back).  CartPole only."""
        capi.check(self._lib.gymnet_vecenv_render_device(self._h, _ptr(d_out), *self._render_args(format, first_lane, count, crop, size, lane_stride)))

    def Render(self, mode="human", lanes=None):
        """CartPoleEnv.Render (CartPoleEnv.cs:69-135): "human" -> None (no viewer); "rgb_array" -> uint8 [len(lanes), 400, 600, 3], the
        full canvas of each lane in `lanes` (default: lane 0 only — a full frame is 720 000 bytes)."""
        if mode == "human":
            return None
        if mode != "rgb_array":
            raise ValueError(f"unsupported render mode {mode!r} (Metadata['render.modes'] = {self.Metadata['render.modes']})")
        lanes = [0] if lanes is None else [int(k) for k in lanes]
        out = np.empty((len(lanes), capi.RENDER_HEIGHT, capi.RENDER_WIDTH, 3), np.uint8)
        for k, lane in enumerate(lanes):
            capi.check(self._lib.gymnet_vecenv_render(self._h, _host(out[k]), *self._render_args("rgb", lane, 1, self._CANVAS, None, None)))
        return out

    def RenderFrames(self, size, crop=_CANVAS, lanes=None):
        """GRAY8 frames of a crop, resized: uint8 [count, out_h, out_w] for the lane range lanes = (first, count) (default: every lane).
        The pixel-input shape of the reference's Images runner is RenderFrames((40, 20), crop=(200, 150, 200, 150))."""
        first, count = (0, self.NumberOfEnvironments) if lanes is None else (int(lanes[0]), int(lanes[1]))
        w, h = int(size[0]), int(size[1])
        out = np.empty((max(count, 0), max(h, 0), max(w, 0)), np.uint8)
        capi.check(self._lib.gymnet_vecenv_render(self._h, _host(out), *self._render_args("gray", first, count, crop, (w, h), None)))
        return out

    def PixelStack(self, depth=2, size=(40, 20), crop=(200, 150, 200, 150), format="binary_f32", out=None):
        """An episode-aware stack of processed frames per lane, kept on the device (gymnet_vecenv_pixel_stack_config): the Images runner's
        2-deep frame queue (ReplayMemory.cs:38-54) and network input (ImageDataBuilder.cs:10-18) with the defaults — two 40 x 20 frames of
        the crop (200, 150, 200, 150), oldest first, 1.0 where a pixel is not background.  format "gray8" / "binary8" (uint8) or
        "binary_f32" (float32).  out=None allocates a torch tensor [N, depth, h, w] on the handle's device; a caller's tensor of that
        dtype is adopted with lane_stride = its stride(0).  Replaces any stack this handle had.  CartPole only."""
        return PixelFrameStack(self, depth, size, crop, format, out)

    def EpisodeMemory(self, capacity=100, max_length=0, history=4, rollout_chunk=0):
        """The trainer's episode memory on the device (gymnet_vecenv_memory_config): every step of each lane's open episode, the best
        `capacity` finished episodes by (return, end tick, lane) and the dataset built from them (ReplayMemory.cs:25-67,
        DataBuilder.cs:25-55).  max_length 0 = the handle's max_episode_steps; history = steps per dataset row (MemoryStates).
        rollout_chunk = C in [1, 64] (gymnet_vecenv_memory_config_rollout) sizes the memory for PushRollout / Rollout passes of C steps:
        C - 1 more staging slots and candidate segments; 0 is the plain config, whose ingest runs one step per pass.  Replaces any memory
        this handle had."""
        return EpisodeMemory(self, capacity, max_length, history, rollout_chunk)

    def Actor(self, net, history=4):
        """A fully connected ReLU network that chooses every lane's action on the device (gymnet_vecenv_actor_config): the trainer's
        ComposeAction -> Trainer.Predict -> argmax (BasePlaySession.cs:78-81) from the last `history` observations of each lane.  net is
        a list of (W, b) pairs (W [out][in], torch's nn.Linear layout) or a torch nn.Sequential of Linear / ReLU layers.  On a Box-action
        env (Pendulum, MountainCarContinuous) it is a Box actor (gymnet_vecenv_actor_box_config): the last layer is one wide and its
        output, clamped to the action bounds, is the action.  Replaces any actor this handle had."""
        return Actor(self, net, history)

    def PackObsDevice(self, d_obs_rowmajor):
        capi.check(self._lib.gymnet_vecenv_pack_obs_device(self._h, _ptr(d_obs_rowmajor)))

    def Sync(self):
        capi.check(self._lib.gymnet_vecenv_sync(self._h))

    def DeviceView(self):
        v = capi.DeviceView()
        capi.check(self._lib.gymnet_vecenv_device_view(self._h, C.byref(v)))
        return v

    def ObsBufferIndex(self):
        """GYMNET_FLAG_DOUBLE_BUFFER: which of the two observation buffers holds the latest observation (0 / 1)."""
        return int(self.DeviceView().obs_buffer)

    def LaunchPolicy(self):
        """The step kernel's launch configuration the handle chose."""
        v, b, nt, sq = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        capi.check(self._lib.gymnet_vecenv_launch_policy(self._h, C.byref(v), C.byref(b), C.byref(nt), C.byref(sq)))
        return {"envs_per_thread": v.value, "block": b.value, "nontemporal_mask": nt.value, "sequential_lanes_per_thread": sq.value}

    _POLICY_FIELDS = ("vec", "block", "nt", "sequential_lanes", "reset_form", "lds_pipe", "occupancy_lds_bytes", "graph")

    def SetLaunchPolicy(self, **fields):
        """gymnet_vecenv_set_launch_policy: override fields of the step kernel's launch configuration (vec, block, nt,
        sequential_lanes, reset_form, lds_pipe, occupancy_lds_bytes, graph; unnamed fields stay).  Every configuration computes
        bit-identical results; a value the handle cannot run raises ValueError.  (This replaces the GYMNET_* environment
        variables of rounds 1-3: the library no longer reads the process environment.)"""
        unknown = set(fields) - set(self._POLICY_FIELDS)
        if unknown:
            raise TypeError(f"unknown launch policy field(s): {sorted(unknown)}")
        p = capi.LaunchPolicy(struct_size=C.sizeof(capi.LaunchPolicy), **{k: int(fields.get(k, -1)) for k in self._POLICY_FIELDS})
        capi.check(self._lib.gymnet_vecenv_set_launch_policy(self._h, C.byref(p)))

    def GetLaunchPolicy(self):
        p = capi.LaunchPolicy()
        capi.check(self._lib.gymnet_vecenv_get_launch_policy(self._h, C.byref(p)))
        return {k: getattr(p, k) for k in self._POLICY_FIELDS}

    def KernelName(self):
        """The template instantiation the next step launch runs, as the launcher itself resolves it
        (e.g. "step_kernel<CartPole,4,true,false,15,1>")."""
        buf = C.create_string_buffer(128)
        capi.check(self._lib.gymnet_vecenv_kernel_name(self._h, buf, 128))
        return buf.value.decode()

    # ---- state access / bookkeeping -----------------------------------------------------------------
    def GetState(self):
        s = np.empty((self.StateDim, self.NumberOfEnvironments), self._dtype)
        capi.check(self._lib.gymnet_vecenv_get_state(self._h, _host(s)))
        return s

    def SetState(self, state_soa):
        s = np.ascontiguousarray(np.asarray(state_soa, dtype=self._dtype))
        if s.shape != (self.StateDim, self.NumberOfEnvironments):
            raise ValueError(f"state must have shape ({self.StateDim}, {self.NumberOfEnvironments})")
        capi.check(self._lib.gymnet_vecenv_set_state(self._h, _host(s)))

    def GetStepsBeyondDone(self):
        b = np.empty(self.NumberOfEnvironments, np.int32)
        capi.check(self._lib.gymnet_vecenv_get_steps_beyond_done(self._h, _host(b)))
        return b

    def SetStepsBeyondDone(self, sbd):
        b = np.ascontiguousarray(np.asarray(sbd, dtype=np.int32))
        if b.shape[0] != self.NumberOfEnvironments:
            raise ValueError("length must equal NumberOfEnvironments")
        capi.check(self._lib.gymnet_vecenv_set_steps_beyond_done(self._h, _host(b)))

    @property
    def Tick(self):
        t = C.c_uint64()
        capi.check(self._lib.gymnet_vecenv_get_tick(self._h, C.byref(t)))
        return t.value

    @Tick.setter
    def Tick(self, value):
        capi.check(self._lib.gymnet_vecenv_set_tick(self._h, int(value)))

    def Counters(self):
        c = capi.Counters()
        capi.check(self._lib.gymnet_vecenv_counters(self._h, C.byref(c)))
        return {"tick": c.tick, "lane_steps": c.lane_steps, "stepped_after_done": c.stepped_after_done,
                "last_done_count": c.last_done_count}

    def DoneLanes(self):
        n = self.NumberOfEnvironments
        lanes = np.empty(n, np.int32)
        cnt = C.c_int64()
        capi.check(self._lib.gymnet_vecenv_done_lanes(self._h, _host(lanes), n, C.byref(cnt)))
        return lanes[:cnt.value].copy()

    def DoneLanesDevice(self, d_lanes_out, d_count_out):
        """Compact list of the lanes that finished in the last step, left on the device (stream-ordered)."""
        capi.check(self._lib.gymnet_vecenv_done_lanes_device(self._h, _ptr(d_lanes_out), _ptr(d_count_out)))

    def DoneRecords(self, episode=None, final_obs=None):
        """Compact records of the lanes that finished in the most recent step (gymnet_vecenv_done_records): dict with
        "lanes" int32 [c] and — by default whenever the handle keeps them — "return" float32 [c], "length" int32 [c],
        "final_obs" [c, D] of the handle's dtype, all in the same (unspecified) order."""
        n = self.NumberOfEnvironments
        episode = self._bookkeeping if episode is None else episode
        final_obs = self._final_obs if final_obs is None else final_obs
        lanes = np.empty(n, np.int32)
        ret = np.empty(n, np.float32) if episode else None
        ln = np.empty(n, np.int32) if episode else None
        fo = np.empty((n, self.ObsDim), self._dtype) if final_obs else None
        cnt = C.c_int64()
        capi.check(self._lib.gymnet_vecenv_done_records(self._h, _host(lanes), None if ret is None else _host(ret), None if ln is None else _host(ln),
                                                        None if fo is None else _host(fo), n, C.byref(cnt)))
        c = cnt.value
        out = {"lanes": lanes[:c].copy()}
        if episode:
            out["return"], out["length"] = ret[:c].copy(), ln[:c].copy()
        if final_obs:
            out["final_obs"] = fo[:c].copy()
        return out

    def DoneRecordsDevice(self, d_lanes, d_return, d_length, d_final_obs, capacity, d_count):
        capi.check(self._lib.gymnet_vecenv_done_records_device(self._h, _ptr(d_lanes), _ptr(d_return), _ptr(d_length), _ptr(d_final_obs),
                                                               int(capacity), _ptr(d_count)))

    def EpisodeStats(self):
        n = self.NumberOfEnvironments
        ret, ln = np.empty(n, np.float32), np.empty(n, np.int32)
        capi.check(self._lib.gymnet_vecenv_episode_stats(self._h, _host(ret), _host(ln)))
        return ret, ln

    def FinalObs(self):
        o = np.empty((self.NumberOfEnvironments, self.ObsDim), self._dtype)
        capi.check(self._lib.gymnet_vecenv_final_obs(self._h, _host(o)))
        return o

    # ---- per-lane arrays by id (gymnet_vecenv_get_array / _set_array) -------------------------------------------------
    _ARRAYS = {"reward": (capi.ARRAY_REWARD, np.float32), "done": (capi.ARRAY_DONE, np.uint8),
               "steps_beyond_done": (capi.ARRAY_STEPS_BEYOND_DONE, np.int32),
               "episode_return": (capi.ARRAY_EPISODE_RETURN, np.float32), "episode_length": (capi.ARRAY_EPISODE_LENGTH, np.int32),
               "finished_return": (capi.ARRAY_FINISHED_RETURN, np.float32), "finished_length": (capi.ARRAY_FINISHED_LENGTH, np.int32),
               "final_obs": (capi.ARRAY_FINAL_OBS, np.float32), "lane_seeds": (capi.ARRAY_LANE_SEEDS, np.uint64)}

    def GetArray(self, name):
        """One of the handle's per-lane arrays by name (see _ARRAYS); "final_obs" is structure-of-arrays [D, N].
        Raises NotImplementedError when the handle's configuration does not keep that array."""
        which, dt = self._ARRAYS[name]
        shape = (self.ObsDim, self.NumberOfEnvironments) if name == "final_obs" else (self.NumberOfEnvironments,)
        if name == "final_obs":
            dt = self._dtype                       # terminal observations carry the handle's state scalar
        a = np.empty(shape, dt)
        capi.check(self._lib.gymnet_vecenv_get_array(self._h, which, _host(a), a.nbytes))
        return a

    def SetArray(self, name, value):
        which, dt = self._ARRAYS[name]
        if name == "final_obs":
            dt = self._dtype
        a = np.ascontiguousarray(np.asarray(value, dtype=dt))
        capi.check(self._lib.gymnet_vecenv_set_array(self._h, which, _host(a), a.nbytes))

    def GetSeed(self):
        """(Philox key in use, whether per-lane keys from Seed(int[]) are active)."""
        s, per = C.c_uint64(), C.c_int32()
        capi.check(self._lib.gymnet_vecenv_get_seed(self._h, C.byref(s), C.byref(per)))
        return s.value, bool(per.value)

    # ---- checkpoint / resume (an extension: the reference has none; everything the engine needs to continue bit for bit) ----
    def Checkpoint(self):
        """EVERY piece of state a handle carries, for ANY configuration (get_state / set_state double as checkpoint /
        resume): the state SoA, the engine tick (the Philox counter word), the seed, and whichever per-lane arrays the handle
        keeps — steps_beyond_done (CartPole without auto-reset), the reward / done flags of the last step (ResetWhere(None)
        consumes them), running episode return / length (they drive the max_episode_steps truncation), the dense
        finished-episode views, terminal observations, the per-lane Philox keys of Seed(int[]).  Restore() on a handle
        created with the same arguments + the same actions reproduce the continuation bit for bit
        (tests/test_gpu_cartpole.py::test_checkpoint_*).  Not part of it: the compacted done LIST of the step before the
        checkpoint (a transient result; DoneLanes() on the restored handle reports none until the next step)."""
        seed, per_lane = self.GetSeed()
        ck = {"env_id": self.EnvId, "num_envs": self.NumberOfEnvironments, "dtype": self._dtype.name, "state": self.GetState(),
              "tick": self.Tick, "seed": seed, "arrays": {}}
        for name in self._ARRAYS:
            if name == "lane_seeds" and not per_lane:
                continue
            try:
                ck["arrays"][name] = self.GetArray(name)
            except NotImplementedError:
                pass                                   # this configuration does not keep that array
        return ck

    def Restore(self, ck):
        if ck["env_id"] != self.EnvId or ck["num_envs"] != self.NumberOfEnvironments or ck.get("dtype", "float32") != self._dtype.name:
            raise ValueError("checkpoint belongs to a different environment / batch size / dtype")
        self.Seed(int(ck["seed"]))                     # also rewinds the tick and drops per-lane keys; both are set again below
        for name, value in ck["arrays"].items():
            self.SetArray(name, value)                 # NotImplementedError: this handle lacks an array the checkpoint carries
        self.SetState(ck["state"])
        self.Tick = ck["tick"]

    # VecEnv.get_attr / set_attr (VecEnv.cs:74-92) select over IEnv objects; here the per-lane
    # attributes that exist are exposed by name.
    def get_attr(self, name):
        if name is None:
            raise ValueError("selector")                       # ArgumentNullException
        if name == "state":
            return self.GetState().T.copy()
        if name == "steps_beyond_done":
            return self.GetStepsBeyondDone()
        raise AttributeError(name)

    def set_attr(self, name, value):
        if value is None:
            raise ValueError("object")                         # ArgumentNullException, VecEnv.cs:88
        if name == "state":
            return self.SetState(np.asarray(value, self._dtype).T)    # the handle's own dtype: float64 state round-trips bit for bit
        if name == "steps_beyond_done":
            return self.SetStepsBeyondDone(value)
        raise AttributeError(name)

    # python-style aliases
    reset, step, seed, close = Reset, Step, Seed, Close


class PixelFrameStack:
    """The handle's pixel stack (VectorEnv.PixelStack).  .Tensor is the device tensor [N, depth, h, w] (the stack itself: read it after
    the handle's stream, e.g. after env.Sync()); Reset / Push / Step are ordered on the handle's stream and do not block."""
    _FORMATS = {"gray8": (capi.STACK_GRAY8, "uint8"), "binary8": (capi.STACK_BINARY8, "uint8"), "binary_f32": (capi.STACK_BINARY_F32, "float32")}

    def __init__(self, env, depth, size, crop, format, out):
        if format not in self._FORMATS:
            raise ValueError(f"unknown pixel stack format {format!r} ({', '.join(self._FORMATS)})")
        import torch
        fmt, dt = self._FORMATS[format]
        w, h = int(size[0]), int(size[1])
        n, depth = env.NumberOfEnvironments, int(depth)
        dtype = getattr(torch, dt)
        if out is None:
            if env.Device is None:
                raise ValueError("this handle's device is not known: pass out=")
            out = torch.empty((n, depth, h, w), dtype=dtype, device=f"cuda:{env.Device}")
            stride = 0
        else:
            if out.dtype != dtype or tuple(out.shape) != (n, depth, h, w) or not out[0].is_contiguous():
                raise ValueError(f"out must be a {dt} tensor [{n}, {depth}, {h}, {w}] whose lanes are contiguous")
            stride = out.stride(0) * out.element_size()
        self._env, self._lib, self._h = env, env._lib, env._h
        self.Format, self.Depth, self.Size, self.Crop = format, depth, (w, h), tuple(int(v) for v in crop)
        capi.check(self._lib.gymnet_vecenv_pixel_stack_config(self._h, fmt, depth, *self.Crop, w, h, _ptr(out), stride))
        prev = getattr(env, "_pixel_stack", None)
        if prev is not None:
            prev._h = None                      # the handle holds one stack: the previous one is gone
        env._pixel_stack = self
        self.Tensor = out

    def _handle(self):
        if self._h is None or not self._env._h:
            raise ValueError("this pixel stack was replaced or closed")
        return self._h

    def Reset(self, mask=None):
        """Every lane whose device mask byte is set (None: every lane) gets its current frame in every slot; after ResetWhere(Device)."""
        capi.check(self._lib.gymnet_vecenv_pixel_stack_reset_device(self._handle(), _ptr(mask)))

    def Push(self, done=None):
        """Once per step: restarting lanes (device done bytes; None: the handle's own with auto_reset, none without) fill every slot with
        the current frame, the others shift by one and take it as the newest."""
        capi.check(self._lib.gymnet_vecenv_pixel_stack_push_device(self._handle(), _ptr(done)))

    def Step(self, d_actions, repeat=0):
        """StepDevice(d_actions) — with repeat > 0 StepRepeatDevice(d_actions, repeat): one decision, the action held for repeat + 1
        env steps — followed by Push().  A lane that finished anywhere inside the decision restarts its stack."""
        repeat = _repeat(repeat)
        if repeat:
            self._env.StepRepeatDevice(d_actions, repeat)
        else:
            self._env.StepDevice(d_actions)
        self.Push()

    def Read(self, lanes=None):
        """The stacks of the lane range lanes = (first, count) (default: every lane) copied to the host: numpy [count, depth, h, w]."""
        first, count = (0, self._env.NumberOfEnvironments) if lanes is None else (int(lanes[0]), int(lanes[1]))
        w, h = self.Size
        out = np.empty((max(count, 0), self.Depth, h, w), np.float32 if self.Format == "binary_f32" else np.uint8)
        capi.check(self._lib.gymnet_vecenv_pixel_stack_read(self._handle(), _host(out), first, count))
        return out

    def Close(self):
        """Releases the stack (the handle stops writing into .Tensor)."""
        if self._h is not None and self._env._h:
            capi.check(self._lib.gymnet_vecenv_pixel_stack_config(self._h, 0, 0, 0, 0, 0, 0, 0, 0, None, 0))
            self._env._pixel_stack = None
        self._h = None


class EpisodeMemory:
    """The handle's episode memory (VectorEnv.EpisodeMemory).  Push / Step / Reset are ordered on the handle's stream and do not block;
    Stats / Episodes / BuildDataset block."""
    _FORMATS = {"params": (capi.MEMORY_PARAMS, "float32"), "gray8": (capi.STACK_GRAY8, "uint8"), "binary8": (capi.STACK_BINARY8, "uint8"),
                "binary_f32": (capi.STACK_BINARY_F32, "float32")}

    def __init__(self, env, capacity, max_length, history, rollout_chunk=0):
        rollout_chunk = _count(rollout_chunk, "rollout_chunk", 0, 64)
        self._env, self._lib, self._h = env, env._lib, env._h
        if rollout_chunk:
            capi.check(self._lib.gymnet_vecenv_memory_config_rollout(self._h, int(capacity), int(max_length), int(history), rollout_chunk))
        else:
            capi.check(self._lib.gymnet_vecenv_memory_config(self._h, int(capacity), int(max_length), int(history)))
        prev = getattr(env, "_episode_memory", None)
        if prev is not None:
            prev._h = None                      # the handle holds one memory: the previous one is gone
        env._episode_memory = self
        self.Capacity, self.History, self.RolloutChunk = int(capacity), int(history), rollout_chunk
        self._rec = None

    def _handle(self):
        if self._h is None or not self._env._h:
            raise ValueError("this episode memory was replaced or closed")
        return self._h

    def Push(self, actions, done=None):
        """Once after each single vector step: the actions that step took (device tensor / pointer) and, optionally, device done bytes
        (None: the handle's own)."""
        capi.check(self._lib.gymnet_vecenv_memory_push_device(self._handle(), _ptr(actions), _ptr(done)))

    def Step(self, actions, repeat=0):
        """StepDevice(actions) — with repeat > 0 StepRepeatDevice(actions, repeat): one decision — followed by Push(actions).  The row of
        a decision is (observation when the action was chosen, action, summed reward, done byte)."""
        repeat = _repeat(repeat)
        if repeat:
            self._env.StepRepeatDevice(actions, repeat)
        else:
            self._env.StepDevice(actions)
        self.Push(actions)

    def PushRollout(self, steps, rec_obs, actions, rec_reward, rec_done, action_stride=None, ring=None):
        """Once after ONE launch of `steps` steps (RolloutFusedDevice with any action source or repeat; StepDevice with steps = 1): the
        rows that launch recorded — rec_obs [T][D][N], rec_reward [T][N], rec_done [T][N] — and its actions, step t's at row
        (t % ring) * action_stride of `actions` (defaults: N and steps, a [T][N] rec_actions; a ring rollout passes its own ring, stride
        and ring length).  The memory ends as `steps` x (StepDevice, Push) would have left it, bit for bit
        (gymnet_vecenv_memory_push_rollout_device)."""
        steps = _count(steps, "steps", 1)
        stride = self._env.NumberOfEnvironments if action_stride is None else _count(action_stride, "action_stride", 0)
        ring = steps if ring is None else _count(ring, "ring", 1)
        capi.check(self._lib.gymnet_vecenv_memory_push_rollout_device(self._handle(), steps, _ptr(rec_obs), _ptr(actions), stride, ring,
                                                                      _ptr(rec_reward), _ptr(rec_done)))

    def Rollout(self, steps, d_actions=None, **rollout_kwargs):
        """RolloutFusedDevice(d_actions, steps, **rollout_kwargs) recording every stream into buffers this memory keeps (and reuses while
        `steps` stays), then PushRollout of them: one rollout launch plus two small launches per rollout_chunk steps.  Returns the
        actions taken: the recorded int32 (Box: float32) torch tensor [steps, N], which the next Rollout overwrites — or, with
        actions="ring", d_actions itself (a ring rollout's actions are its ring)."""
        import torch
        steps = _count(steps, "steps", 1)
        env = self._env
        self._handle()
        taken = set(rollout_kwargs) & {"rec_obs", "rec_reward", "rec_done", "rec_actions"}
        if taken:
            raise TypeError(f"Rollout records into its own buffers: {sorted(taken)}")
        if env.Device is None:
            raise ValueError("this handle's device is not known")
        n, box = env.NumberOfEnvironments, isinstance(env.ActionSpace, Box)
        if self._rec is None or self._rec[0].shape[0] != steps:
            dev = f"cuda:{env.Device}"
            self._rec = (torch.empty((steps, env.ObsDim, n), dtype=getattr(torch, env._dtype.name), device=dev),
                         torch.empty((steps, n), dtype=torch.float32, device=dev), torch.empty((steps, n), dtype=torch.uint8, device=dev),
                         torch.empty((steps, n), dtype=torch.float32 if box else torch.int32, device=dev))
        obs, rew, done, act = self._rec
        if rollout_kwargs.get("actions", "ring") == "ring":       # a ring rollout's actions ARE its ring: nothing to record
            if d_actions is None:              # (checked before the launch: a refused ingest after it would leave the memory behind)
                raise ValueError("a ring rollout needs d_actions")
            env.RolloutFusedDevice(d_actions, steps, rec_obs=obs, rec_reward=rew, rec_done=done, **rollout_kwargs)
            self.PushRollout(steps, obs, d_actions, rew, done, action_stride=rollout_kwargs.get("action_stride", 0),
                             ring=rollout_kwargs.get("ring", 1))
            return d_actions
        env.RolloutFusedDevice(d_actions, steps, rec_obs=obs, rec_reward=rew, rec_done=done, rec_actions=act, **rollout_kwargs)
        self.PushRollout(steps, obs, act, rew, done)
        return act

    def Reset(self, mask=None, clear=False):
        """Lanes whose device mask byte is set (None: every lane) open a new episode from their current observation (after
        ResetWhere(Device)); clear=True also empties the pool and zeroes the counters."""
        capi.check(self._lib.gymnet_vecenv_memory_reset_device(self._handle(), _ptr(mask), 1 if clear else 0))

    def Stats(self):
        """dict kept / ended / admitted / too_long."""
        v = [C.c_int64() for _ in range(4)]
        capi.check(self._lib.gymnet_vecenv_memory_stats(self._handle(), *(C.byref(x) for x in v)))
        return dict(zip(("kept", "ended", "admitted", "too_long"), (int(x.value) for x in v)))

    def Episodes(self):
        """The kept episodes in descending key order: numpy arrays (return float32, length int32, end_tick uint64, lane int32)."""
        count = C.c_int64()
        capi.check(self._lib.gymnet_vecenv_memory_episodes(self._handle(), None, None, None, None, 0, C.byref(count)))
        k = int(count.value)
        ret, ln, tick, lane = np.empty(k, np.float32), np.empty(k, np.int32), np.empty(k, np.uint64), np.empty(k, np.int32)
        capi.check(self._lib.gymnet_vecenv_memory_episodes(self._handle(), _host(ret), _host(ln), _host(tick), _host(lane), k, C.byref(count)))
        return ret, ln, tick, lane

    def DatasetSize(self):
        rows = C.c_int64()
        capi.check(self._lib.gymnet_vecenv_memory_dataset_size(self._handle(), C.byref(rows)))
        return int(rows.value)

    def BuildDataset(self, format="params", size=(40, 20), crop=(200, 150, 200, 150), min_episodes=None, reward=False):
        """DataBuilder.BuildDataset on the device: torch tensors (x, action, onehot) on the handle's device, or None while fewer than
        min_episodes (default: the capacity) episodes are kept.  x is float32 [rows, history * obs_dim] for "params", else
        [rows, history, h, w] frames ("gray8" / "binary8" uint8, "binary_f32" float32; CartPole only).  onehot is None for a Box
        action.  reward=True appends the rewards (float32 [rows])."""
        if format not in self._FORMATS:
            raise ValueError(f"unknown dataset format {format!r} ({', '.join(self._FORMATS)})")
        import torch
        env = self._env
        if env.Device is None:
            raise ValueError("this handle's device is not known")
        if self.Stats()["kept"] < (self.Capacity if min_episodes is None else int(min_episodes)):
            return None
        fmt, dt = self._FORMATS[format]
        rows = self.DatasetSize()
        dev = f"cuda:{env.Device}"
        w, h = int(size[0]), int(size[1])
        shape = (rows, self.History * env.ObsDim) if fmt == capi.MEMORY_PARAMS else (rows, self.History, h, w)
        x = torch.empty(shape, dtype=getattr(torch, dt), device=dev)
        action = torch.empty(rows, dtype=torch.float32 if isinstance(env.ActionSpace, Box) else torch.int32, device=dev)
        onehot = None if isinstance(env.ActionSpace, Box) else torch.empty((rows, env.ActionSpace.N), dtype=torch.float32, device=dev)
        rew = torch.empty(rows, dtype=torch.float32, device=dev) if reward else None
        cx, cy, cw, ch = (int(v) for v in crop)
        capi.check(self._lib.gymnet_vecenv_memory_dataset_device(self._handle(), fmt, cx, cy, cw, ch, w, h, _ptr(x), _ptr(action),
                                                                 _ptr(onehot), _ptr(rew), rows))
        env.Sync()
        return (x, action, onehot, rew) if reward else (x, action, onehot)

    def Close(self):
        """Releases the memory."""
        if self._h is not None and self._env._h:
            capi.check(self._lib.gymnet_vecenv_memory_config(self._h, 0, 0, 0))
            self._env._episode_memory = None
        self._h = None


def actor_layers(net):
    """[(W float32 [out][in], b float32 [out]), ...] from a list of (W, b) pairs or a torch nn.Sequential of Linear / ReLU layers (every
    Linear but the last followed by one ReLU, the last by none)."""
    if hasattr(net, "named_children") or hasattr(net, "children"):
        import torch
        mods = list(net.children())
        layers, expect_relu = [], False
        for m in mods:
            if isinstance(m, torch.nn.Linear):
                if expect_relu:
                    raise ValueError("every Linear layer but the last must be followed by a ReLU")
                w = m.weight.detach().to("cpu", torch.float32).numpy()
                b = (m.bias.detach().to("cpu", torch.float32).numpy() if m.bias is not None else np.zeros(w.shape[0], np.float32))
                layers.append((w, b))
                expect_relu = True
            elif isinstance(m, torch.nn.ReLU):
                if not expect_relu:
                    raise ValueError("a ReLU must follow a Linear layer")
                expect_relu = False
            else:
                raise ValueError(f"unsupported layer {type(m).__name__} (Linear / ReLU only)")
        if not layers or not expect_relu:
            raise ValueError("the network must end with a Linear layer (its outputs are the logits)")
        return layers
    out = []
    for pair in net:
        w, b = pair
        w = np.ascontiguousarray(np.asarray(w.detach().cpu() if hasattr(w, "detach") else w, np.float32))
        b = np.ascontiguousarray(np.asarray(b.detach().cpu() if hasattr(b, "detach") else b, np.float32))
        if w.ndim != 2 or b.shape != (w.shape[0],):
            raise ValueError(f"layer {len(out)}: W must be [out][in] and b [out], got {w.shape} and {b.shape}")
        out.append((w, b))
    if not out:
        raise ValueError("the network has no layer")
    return out


def actor_pack(net, box=False):
    """(widths int32 [L + 1], weights float32 [count]) in gymnet_vecenv_actor_config's layout: per layer W row-major, then b.  box: the
    network of a Box actor (gymnet_vecenv_actor_box_config), whose last layer must be one wide."""
    layers = actor_layers(net)
    if box and layers[-1][0].shape[0] != 1:
        raise ValueError(f"a Box actor's last layer gives the one action value; this one is {layers[-1][0].shape[0]} wide")
    widths = [layers[0][0].shape[1]]
    for k, (w, b) in enumerate(layers):
        if w.shape[1] != widths[-1]:
            raise ValueError(f"layer {k} takes {w.shape[1]} inputs, the previous layer gives {widths[-1]}")
        widths.append(w.shape[0])
    flat = np.concatenate([np.concatenate([w.reshape(-1), b]) for w, b in layers]).astype(np.float32)
    return np.asarray(widths, np.int32), flat


class Actor:
    """The handle's actor (VectorEnv.Actor).  Act / Push / Reset / Load / Step are ordered on the handle's stream and do not block;
    History blocks."""

    def __init__(self, env, net, history):
        history = int(history)
        self.IsBox = isinstance(env.ActionSpace, Box)
        widths, flat = actor_pack(net, box=self.IsBox)
        if history < 1:
            raise ValueError("history must be >= 1")
        if widths[0] != history * env.ObsDim:
            raise ValueError(f"the first layer takes {widths[0]} inputs; history * obs_dim = {history * env.ObsDim}")
        self._env, self._lib, self._h = env, env._lib, env._h
        config = self._lib.gymnet_vecenv_actor_box_config if self.IsBox else self._lib.gymnet_vecenv_actor_config
        capi.check(config(self._h, history, len(widths) - 1, _host(widths), _host(flat), flat.size))
        prev = getattr(env, "_actor", None)
        if prev is not None and prev is not self:
            prev._h = None                      # the handle holds one actor: the previous one is gone
        env._actor = self
        self.History_, self.Widths, self.Count = history, tuple(int(w) for w in widths), int(flat.size)
        self.CriticWidths, self.CriticCount = None, 0          # (a new actor has no critic: the config call dropped it)
        self._out = None

    def _handle(self):
        if self._h is None or not self._env._h:
            raise ValueError("this actor was replaced or closed")
        return self._h

    def _critic_pack(self, net):
        """actor_pack of a critic's network, its first and last width checked against this actor before any native call"""
        widths, flat = actor_pack(net)
        if int(widths[0]) != self.Widths[0]:
            raise ValueError(f"the critic's first layer takes {int(widths[0])} inputs; the actor's input is history * obs_dim = {self.Widths[0]}")
        if int(widths[-1]) != 1:
            raise ValueError(f"the critic's last layer gives the one value; this one is {int(widths[-1])} wide")
        return widths, flat

    def SetCritic(self, net):
        """Attaches a critic (gymnet_vecenv_actor_critic_config): a second network — an nn.Sequential of Linear / ReLU layers or (W, b)
        pairs, as VectorEnv.Actor takes — over the input this actor reads, history * obs_dim wide, whose last layer is one wide: the
        lane's value.  Depth and hidden widths are its own.  None removes it.  Either kind of actor takes one; a new VectorEnv.Actor
        drops it; Load, Push, Reset, SetExploration and SetPolicy keep it."""
        if net is None:
            capi.check(self._lib.gymnet_vecenv_actor_critic_config(self._handle(), 0, None, None, 0))
            self.CriticWidths, self.CriticCount = None, 0
            return
        widths, flat = self._critic_pack(net)
        capi.check(self._lib.gymnet_vecenv_actor_critic_config(self._handle(), len(widths) - 1, _host(widths), _host(flat), flat.size))
        self.CriticWidths, self.CriticCount = tuple(int(w) for w in widths), int(flat.size)

    def LoadCritic(self, net):
        """New critic weights of the configured widths (gymnet_vecenv_actor_critic_load_device), as Load takes the actor's: a flat device
        float32 tensor in the config layout is copied device to device, anything else goes through actor_pack and the host."""
        if getattr(self, "CriticWidths", None) is None:
            raise ValueError("this actor has no critic (SetCritic)")
        if hasattr(net, "data_ptr") and getattr(net, "is_cuda", False):
            if net.numel() != self.CriticCount or str(net.dtype) != "torch.float32" or not net.is_contiguous():
                raise ValueError(f"a device weight tensor must be {self.CriticCount} contiguous float32 values")
            capi.check(self._lib.gymnet_vecenv_actor_critic_load_device(self._handle(), _ptr(net), self.CriticCount))
            return
        widths, flat = self._critic_pack(net)
        if tuple(int(w) for w in widths) != self.CriticWidths:
            raise ValueError(f"widths {tuple(int(w) for w in widths)} != the critic's {self.CriticWidths}")
        import torch
        d = torch.from_numpy(flat).to(f"cuda:{self._env.Device}")
        capi.check(self._lib.gymnet_vecenv_actor_critic_load_device(self._handle(), _ptr(d), self.CriticCount))
        self._env.Sync()

    def _value_buffer(self, value, name="value"):
        if getattr(self, "CriticWidths", None) is None:
            raise ValueError(f"{name} needs a critic (SetCritic)")
        return _logp_buffer(value, (self._env.NumberOfEnvironments,), name, self._env.Device)

    def Value(self, out=None):
        """The critic's value of every lane's current history into `out` (device float32 [N]; None: a new torch tensor, returned), one
        kernel on the handle's stream (gymnet_vecenv_actor_value_device).  Serves Box actors and float64 handles too; the history must be
        current, as for Act.  After a rollout this is the last value."""
        if out is None:
            if getattr(self, "CriticWidths", None) is None:
                raise ValueError("value needs a critic (SetCritic)")
            import torch
            out = torch.empty(self._env.NumberOfEnvironments, dtype=torch.float32, device=f"cuda:{self._env.Device}")
        else:
            self._value_buffer(out, "out")
        capi.check(self._lib.gymnet_vecenv_actor_value_device(self._handle(), _ptr(out)))
        return out

    def Boot(self, out=None):
        """V(terminal observation) of every lane whose done byte has bit 1 set (a time limit), +0.0 for every other lane, into `out`
        (device float32 [N]; None: a new torch tensor, returned): one row of AdvantagesDevice's boot= (gymnet_vecenv_actor_boot_device).
        Call it after a vector step and before Push.  The terminal observation is read from the dense final observations on an
        auto_reset handle (final_obs=True) and from the current observation otherwise; the handle needs max_episode_steps > 0.  Changes
        neither the history nor what Push does next."""
        if out is None:
            if getattr(self, "CriticWidths", None) is None:
                raise ValueError("boot needs a critic (SetCritic)")
            import torch
            out = torch.empty(self._env.NumberOfEnvironments, dtype=torch.float32, device=f"cuda:{self._env.Device}")
        else:
            self._value_buffer(out, "out")
        capi.check(self._lib.gymnet_vecenv_actor_boot_device(self._handle(), _ptr(out)))
        return out

    def Act(self, epsilon=0.0, seed=0, tick=0, out=None, logits=None, logp=None, value=None, logd=None):
        """Every lane's action into `out` (device int32 [N]; None: a torch tensor on the handle's device, returned): the argmax of the
        network's logits over the lane's history, epsilon-greedy as ComposeActionsDevice(greedy, epsilon, seed=seed, tick=tick) would
        compose it.  logits: an optional device float32 [N, action_n].  A Box actor (gymnet_vecenv_actor_box_act_device): `out` is
        float32 [N] — the network's one output clamped to the action bounds, or ActionSpace.Sample() as SampleActionsDevice(seed=seed,
        tick=tick) draws it where the lane explores — and logits takes the [N, 1] unclamped outputs.  That is the default policy;
        SetPolicy changes the head and what an exploring lane takes.  On a Discrete actor SetExploration("softmax", temperature) makes an
        exploring lane draw from softmax(logits / temperature) instead.  logp (a Discrete actor): an optional device float32 [N] for the
        log-probability of the action each lane takes under softmax(logits / temperature), the stored temperature whatever the exploration
        setting (gymnet_vecenv_actor_act_logp_device); actions and logits are the same bits with and without it.  value (a Discrete actor
        with a critic): an optional device float32 [N] for what Value() writes, from the same call
        (gymnet_vecenv_actor_act_value_device); actions, logits and logp are the same bits with and without it.  logd (a Box actor whose
        policy has sigma > 0): an optional device float32 [N] for the log-density log N(action; greedy action, sigma^2) of the action each
        lane takes (gymnet_vecenv_actor_box_act_logd_device); actions and the unclamped outputs are the same bits with and without it."""
        if logd is not None:
            if not self.IsBox:
                raise ValueError("logd belongs to a Box actor; this one chooses Discrete actions (logp)")
            _logp_buffer(logd, (self._env.NumberOfEnvironments,), "logd", self._env.Device)
        if logp is not None:
            if self.IsBox:
                raise ValueError("logp belongs to a Discrete actor; this one chooses Box actions")
            _logp_buffer(logp, (self._env.NumberOfEnvironments,), "logp", self._env.Device)
        if value is not None:
            if self.IsBox:
                raise ValueError("Act(value=) belongs to a Discrete actor; this one chooses Box actions (Value() serves it)")
            self._value_buffer(value)
        if out is None:
            out = self._actions()
        if logd is not None:
            capi.check(self._lib.gymnet_vecenv_actor_box_act_logd_device(self._handle(), _ptr(out), _ptr(logits), _ptr(logd), float(epsilon),
                                                                         int(seed) & 0xFFFFFFFFFFFFFFFF, int(tick)))
            return out
        if value is not None:
            capi.check(self._lib.gymnet_vecenv_actor_act_value_device(self._handle(), _ptr(out), _ptr(logits), _ptr(logp), _ptr(value), float(epsilon),
                                                                      int(seed) & 0xFFFFFFFFFFFFFFFF, int(tick)))
            return out
        if logp is not None:
            capi.check(self._lib.gymnet_vecenv_actor_act_logp_device(self._handle(), _ptr(out), _ptr(logits), _ptr(logp), float(epsilon),
                                                                     int(seed) & 0xFFFFFFFFFFFFFFFF, int(tick)))
            return out
        act = self._lib.gymnet_vecenv_actor_box_act_device if self.IsBox else self._lib.gymnet_vecenv_actor_act_device
        capi.check(act(self._handle(), _ptr(out), _ptr(logits), float(epsilon), int(seed) & 0xFFFFFFFFFFFFFFFF, int(tick)))
        return out

    _HEADS = {"clamp": capi.BOX_HEAD_CLAMP, "tanh": capi.BOX_HEAD_TANH}
    _EXPLORES = {"sample": capi.BOX_EXPLORE_SAMPLE, "gaussian": capi.BOX_EXPLORE_GAUSSIAN}

    def SetPolicy(self, head="clamp", explore="sample", sigma=0.0):
        """A Box actor's policy (gymnet_vecenv_actor_box_set_policy), read by Act, Step and RolloutFusedDevice(actions="actor") from the
        next call on.  head: "clamp" (the network's output clamped to the bounds) or "tanh" (mid + half * tanh(output)).  explore: what
        a lane whose coin says "explore" takes: "sample" (ActionSpace.Sample()) or "gaussian" (the greedy action plus sigma * a standard
        normal draw, clamped to the bounds).  A new actor has ("clamp", "sample", 0.0); Load, Push and Reset keep the policy."""
        if not self.IsBox:
            raise ValueError("a policy belongs to a Box actor; this one chooses Discrete actions")
        if head not in self._HEADS:
            raise ValueError(f"head must be one of {sorted(self._HEADS)}, got {head!r}")
        if explore not in self._EXPLORES:
            raise ValueError(f"explore must be one of {sorted(self._EXPLORES)}, got {explore!r}")
        sigma = float(sigma)
        if not (np.isfinite(sigma) and sigma >= 0.0):
            raise ValueError("sigma must be finite and >= 0")
        capi.check(self._lib.gymnet_vecenv_actor_box_set_policy(self._handle(), self._HEADS[head], self._EXPLORES[explore], sigma))

    @property
    def Policy(self):
        """(head, explore, sigma) as SetPolicy takes them, read from the library (gymnet_vecenv_actor_box_get_policy)."""
        if not self.IsBox:
            raise ValueError("a policy belongs to a Box actor; this one chooses Discrete actions")
        head, explore, sigma = C.c_int32(), C.c_int32(), C.c_float()
        capi.check(self._lib.gymnet_vecenv_actor_box_get_policy(self._handle(), C.byref(head), C.byref(explore), C.byref(sigma)))
        heads, explores = {v: k for k, v in self._HEADS.items()}, {v: k for k, v in self._EXPLORES.items()}
        return heads[head.value], explores[explore.value], float(sigma.value)

    _EXPLORATIONS = {"uniform": capi.ACTOR_EXPLORE_UNIFORM, "softmax": capi.ACTOR_EXPLORE_SOFTMAX}

    def SetExploration(self, explore="uniform", temperature=1.0):
        """A Discrete actor's exploration setting (gymnet_vecenv_actor_set_exploration), read by Act, Step, RolloutFusedDevice(actions=
        "actor") and EpisodeMemory.Rollout(actions="actor") from the next call on.  explore: what a lane whose coin says "explore" takes:
        "uniform" (ActionSpace.Sample()) or "softmax" (a draw from softmax(logits / temperature): at epsilon = 1 every lane samples the
        stochastic policy).  A new actor has ("uniform", 1.0); Load, Push and Reset keep the setting."""
        if self.IsBox:
            raise ValueError("an exploration setting belongs to a Discrete actor; this one chooses Box actions (SetPolicy)")
        if not isinstance(explore, str) or explore not in self._EXPLORATIONS:
            raise ValueError(f"explore must be one of {sorted(self._EXPLORATIONS)}, got {explore!r}")
        if isinstance(temperature, (bool, np.bool_)):
            raise ValueError("temperature must be a number, not a bool")
        with np.errstate(over="ignore", divide="ignore"):
            temperature = float(np.float32(temperature))
            ok = np.isfinite(temperature) and temperature > 0.0 and np.isfinite(np.float32(1.0) / np.float32(temperature))
        if not ok:
            raise ValueError("temperature must be finite, > 0 and large enough for a finite float32 1 / temperature")
        capi.check(self._lib.gymnet_vecenv_actor_set_exploration(self._handle(), self._EXPLORATIONS[explore], temperature))

    @property
    def Exploration(self):
        """(explore, temperature) as SetExploration takes them, read from the library (gymnet_vecenv_actor_get_exploration)."""
        if self.IsBox:
            raise ValueError("an exploration setting belongs to a Discrete actor; this one chooses Box actions (Policy)")
        explore, temperature = C.c_int32(), C.c_float()
        capi.check(self._lib.gymnet_vecenv_actor_get_exploration(self._handle(), C.byref(explore), C.byref(temperature)))
        return {v: k for k, v in self._EXPLORATIONS.items()}[explore.value], float(temperature.value)

    def _actions(self):
        import torch
        return torch.empty(self._env.NumberOfEnvironments, dtype=torch.float32 if self.IsBox else torch.int32, device=f"cuda:{self._env.Device}")

    def Push(self, done=None):
        """Once after each single vector step: lanes whose done byte is set (device bytes; None: the handle's own) refill every slot with
        their post-step observation, the others append it."""
        capi.check(self._lib.gymnet_vecenv_actor_push_device(self._handle(), _ptr(done)))

    def Reset(self, mask=None):
        """Lanes whose device mask byte is set (None: every lane) fill every slot with their current observation (after ResetWhere(Device))."""
        capi.check(self._lib.gymnet_vecenv_actor_reset_device(self._handle(), _ptr(mask)))

    def Load(self, net):
        """New weights of the same widths, history kept: a flat device float32 tensor in the config layout is copied device to device,
        anything else goes through actor_pack and the host."""
        if hasattr(net, "data_ptr") and getattr(net, "is_cuda", False):
            if net.numel() != self.Count or str(net.dtype) != "torch.float32" or not net.is_contiguous():
                raise ValueError(f"a device weight tensor must be {self.Count} contiguous float32 values")
            capi.check(self._lib.gymnet_vecenv_actor_load_device(self._handle(), _ptr(net), self.Count))
            return
        widths, flat = actor_pack(net)
        if tuple(int(w) for w in widths) != self.Widths:
            raise ValueError(f"widths {tuple(int(w) for w in widths)} != the actor's {self.Widths}")
        import torch
        d = torch.from_numpy(flat).to(f"cuda:{self._env.Device}")
        capi.check(self._lib.gymnet_vecenv_actor_load_device(self._handle(), _ptr(d), self.Count))
        self._env.Sync()

    def History(self):
        """numpy float32 [N, history, obs_dim], oldest first (blocks)."""
        p, stride, slot = C.c_void_p(), C.c_int64(), C.c_int32()
        capi.check(self._lib.gymnet_vecenv_actor_view(self._handle(), C.byref(p), C.byref(stride), C.byref(slot)))
        import torch
        env = self._env
        env.Sync()
        n, S, O = env.NumberOfEnvironments, self.History_, env.ObsDim

        class _View:                            # the library's history buffer, seen by torch without a copy
            __cuda_array_interface__ = {"shape": (S, O, int(stride.value)), "typestr": "<f4", "data": (int(p.value or 0), False),
                                        "version": 2, "strides": None}
        raw = torch.as_tensor(_View(), device=f"cuda:{env.Device}").cpu().numpy()[:, :, :n]
        order = [(int(slot.value) + 1 + s) % S for s in range(S)]
        return np.ascontiguousarray(raw[order].transpose(2, 0, 1))

    def HistoryDevice(self, out=None):
        """The history as a torch float32 [history, obs_dim, N] on the device, oldest first (gymnet_vecenv_actor_history_device): a copy
        on the handle's stream that does not block, and that a later Push or rollout does not overwrite.  Taken before
        RolloutFusedDevice(actions="actor") it is the history0 of VectorEnv.RolloutInputsDevice.  out: a caller-allocated tensor of
        that shape; None: a new one.  The history must be current, as for Act."""
        env = self._env
        shape = (self.History_, env.ObsDim, env.NumberOfEnvironments)
        if out is None:
            import torch
            out = torch.empty(shape, dtype=torch.float32, device=f"cuda:{env.Device}")
        else:
            _logp_buffer(out, shape, "out", env.Device)
        capi.check(self._lib.gymnet_vecenv_actor_history_device(self._handle(), _ptr(out), env.NumberOfEnvironments))
        return out

    def Step(self, epsilon=0.0, seed=0, tick=0, repeat=0, logp=None, value=None, logd=None, boot=None):
        """Act(epsilon, seed, tick, logp=logp, value=value, logd=logd), StepDevice — with repeat > 0 StepRepeatDevice: the action held for repeat + 1 env steps —,
        Push(): one closed-loop decision; returns the device actions taken.  boot: an optional device float32 [N] that takes Boot()
        between the step and the push."""
        repeat = _repeat(repeat)
        if logp is not None and self.IsBox:
            raise ValueError("logp belongs to a Discrete actor; this one chooses Box actions")
        if value is not None and self.IsBox:
            raise ValueError("Step(value=) belongs to a Discrete actor; this one chooses Box actions (Value() serves it)")
        if logd is not None and not self.IsBox:
            raise ValueError("logd belongs to a Box actor; this one chooses Discrete actions (logp)")
        if boot is not None:
            self._value_buffer(boot, "boot")
        if self._out is None:
            self._out = self._actions()
        self.Act(epsilon, seed, tick, out=self._out, logp=logp, value=value, logd=logd)
        if repeat:
            self._env.StepRepeatDevice(self._out, repeat)
        else:
            self._env.StepDevice(self._out)
        if boot is not None:
            self.Boot(boot)
        self.Push()
        return self._out

    def Close(self):
        """Releases the actor."""
        if self._h is not None and self._env._h:
            capi.check(self._lib.gymnet_vecenv_actor_config(self._h, 0, 0, None, None, 0))      # (releases either kind)
            self._env._actor = None
        self._h = None


class GroupVectorEnv:
    """One process driving G GPUs (or G logical members on one GPU): the ctypes mirror of gymnet_group_* — what a
    P/Invoking C# host uses instead of torch.distributed.  Member m owns global lanes [m*N/G, (m+1)*N/G); every member
    keeps a replica [G][D][N/G] of all observations on its GPU, completed by AllGatherObs() (hand-written direct push over
    peer-mapped memory, or RCCL).  Same VecEnv surface for the host-boundary path (Reset / Step over the whole batch)."""

    def __init__(self, env="CartPole-v1", global_num_envs=1, num_members=1, devices=None, seed=0, auto_reset=False,
                 gather="direct", overlap=False, validate_actions=False, max_episode_steps=0, episode_stats=False, dtype=np.float32):
        """dtype=np.float64 (CartPole): every member runs GYMNET_FLAG_F64 — the reference's own arithmetic — and the replicas,
        the gather and the host batches carry doubles."""
        env_id = capi.ENV_IDS[env] if isinstance(env, str) else int(env)
        self._lib = capi.load_library()
        self._dtype = np.dtype(dtype)
        if self._dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("dtype must be float32 or float64")
        flags = ((capi.FLAG_AUTORESET if auto_reset else 0) | (capi.FLAG_VALIDATE_ACTIONS if validate_actions else 0)
                 | (capi.FLAG_DOUBLE_BUFFER if overlap else 0) | (capi.FLAG_EPISODE_STATS if episode_stats else 0)
                 | (capi.FLAG_F64 if self._dtype == np.float64 else 0))
        mode = {"none": capi.GATHER_NONE, "direct": capi.GATHER_DIRECT, "rccl": capi.GATHER_RCCL}[gather] if isinstance(gather, str) else int(gather)
        devs = None
        if devices is not None:
            if len(devices) != num_members:
                raise ValueError("len(devices) must equal num_members")
            devs = (C.c_int32 * num_members)(*[int(d) for d in devices])
        cfg = capi.GroupConfig(struct_size=C.sizeof(capi.GroupConfig), env_id=env_id, global_num_envs=int(global_num_envs),
                               num_members=int(num_members), flags=flags, seed=int(seed) & 0xFFFFFFFFFFFFFFFF,
                               devices=devs, gather=mode, max_episode_steps=int(max_episode_steps))
        self._g = C.c_void_p()
        capi.check(self._lib.gymnet_group_create(C.byref(cfg), C.byref(self._g)))
        info = capi.env_describe(env_id)
        self.NumberOfEnvironments = int(global_num_envs)
        self.NumMembers = int(num_members)
        self.LanesPerMember = int(global_num_envs) // int(num_members)
        self.ObsDim = int(info.obs_dim)
        self.Overlap = bool(overlap)
        self.Members = []
        for m in range(self.NumMembers):
            h = C.c_void_p()
            capi.check(self._lib.gymnet_group_member(self._g, m, C.byref(h)))
            self.Members.append(VectorEnv._borrow(h, env_id, self.LanesPerMember, auto_reset, self._dtype))
        self.ActionSpace, self.ObservationSpace = self.Members[0].ActionSpace, self.Members[0].ObservationSpace
        self.Metadata, self.RewardRange = self.Members[0].Metadata, self.Members[0].RewardRange
        self._adtype = self.Members[0]._adtype
        self.Environments = []

    def Close(self):
        if getattr(self, "_g", None) is not None and self._g:
            for m in self.Members:
                m.Close()
            self._lib.gymnet_group_destroy(self._g)
            self._g = C.c_void_p()

    Dispose = Close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.Close()

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass

    def Seed(self, seed):
        capi.check(self._lib.gymnet_group_seed(self._g, int(seed) & 0xFFFFFFFFFFFFFFFF))

    # host-boundary path over the whole batch
    def Reset(self):
        obs = np.empty((self.NumberOfEnvironments, self.ObsDim), self._dtype)
        capi.check(self._lib.gymnet_group_reset(self._g, _host(obs)))
        return obs

    def Step(self, action):
        n = self.NumberOfEnvironments
        if isinstance(action, enum.Enum):
            action = int(action.value)
        if isinstance(action, (int, np.integer)) and not isinstance(action, (bool, np.bool_)):
            action = np.full(n, action, dtype=self._adtype)                          # IVecEnv.Step(int): broadcast
        a = np.ascontiguousarray(np.asarray(action).reshape(-1).astype(self._adtype, copy=False))
        if a.shape[0] != n:
            raise ValueError("Number of actions passed should be equals to number of environments")
        obs, rew, done = np.empty((n, self.ObsDim), self._dtype), np.empty(n, np.float32), np.empty(n, np.uint8)
        capi.check(self._lib.gymnet_group_step(self._g, _host(a), _host(obs), _host(rew), _host(done)))
        return BatchStep(obs, rew, done.astype(bool), None, truncated=(done & 2) != 0)

    # device-resident path
    def ResetDevice(self):
        capi.check(self._lib.gymnet_group_reset_device(self._g))

    def _ptrs(self, d_actions):
        if len(d_actions) != self.NumMembers:
            raise ValueError("one device pointer per member")
        return (C.c_void_p * self.NumMembers)(*[_ptr(p) for p in d_actions])

    def StepDevice(self, d_actions):
        capi.check(self._lib.gymnet_group_step_device(self._g, self._ptrs(d_actions)))

    def RolloutDevice(self, d_actions, steps, action_stride, ring):
        capi.check(self._lib.gymnet_group_rollout_device(self._g, self._ptrs(d_actions), int(steps), int(action_stride), int(ring)))

    def AllGatherObs(self):
        capi.check(self._lib.gymnet_group_allgather_obs(self._g))

    def WaitGather(self):
        capi.check(self._lib.gymnet_group_wait_gather(self._g))

    def GlobalObsPtr(self, member):
        p = C.c_void_p()
        capi.check(self._lib.gymnet_group_global_obs(self._g, int(member), C.byref(p)))
        return p.value

    def ReadReplica(self, member):
        """Member's replica of all observations on the host, [G, D, N/G] (waits for the last gather)."""
        out = np.empty((self.NumMembers, self.ObsDim, self.LanesPerMember), self._dtype)
        capi.check(self._lib.gymnet_group_read_replica(self._g, int(member), _host(out)))
        return out

    def Sync(self):
        capi.check(self._lib.gymnet_group_sync(self._g))

    reset, step, seed, close = Reset, Step, Seed, Close


class DummyVecEnv(VectorEnv):
    """DummyVecEnv (src/Gym/Envs/DummyVecEnv.cs:2-4): a VecEnv around ONE environment — here a 1-lane batch."""

    def __init__(self, env="CartPole-v1", **kw):
        super().__init__(env, 1, **kw)


class GpuEnv:
    """Single-instance `Env` façade (Env.cs:13-41) over a 1-lane VectorEnv: Reset() -> NDArray[D],
    Step(object action) -> Step.  Exists so an existing per-instance loop (README.md:32-52,
    tests/Gym.Tests/Envs/Classic/CartpoleEnvironment.cs:14-35) runs unmodified on the engine."""
    ENV = "CartPole-v1"
    DTYPE = np.float32          # CartPoleEnv overrides: float64, the reference's own arithmetic

    def __init__(self, device=0, seed=0, validate_actions=False, max_episode_steps=0, dtype=None, resident=False):
        """max_episode_steps > 0 adds the TimeLimit wrapper upstream gym registers with the env (500 / 200; an extension: the
        reference has no time limit): the step that reaches the limit returns Done with
        Information["TimeLimit.truncated"] = True — the same shape as the C# GpuEnv (csharp/GpuEnv.cs).
        resident=True (opt-in since round 6): Step / Reset go through GYMNET_FLAG_RESIDENT — a resident single-wave kernel polling
        a mailbox in pinned host memory — instead of a kernel launch + synchronize per call: ~3x lower latency for a loop that does
        nothing but step (README.md:32-52), bit-identical results.  The price: while the kernel waits for the next command it occupies
        the handle's stream for up to ~5 ms, and a device-wide synchronize elsewhere in the process (torch.cuda.synchronize(), a
        caching allocator's hipFree) or serialised dispatch (rocprofv3 --pmc) waits for that — so a process that also trains on the
        GPU keeps the default, one launch per call."""
        self._v = VectorEnv(self.ENV, 1, device=device, seed=seed, auto_reset=False, validate_actions=validate_actions,
                            episode_stats=max_episode_steps > 0, max_episode_steps=max_episode_steps,
                            dtype=self.DTYPE if dtype is None else dtype, resident=resident)
        self.ActionSpace, self.ObservationSpace = self._v.ActionSpace, self._v.ObservationSpace
        self.Metadata, self.RewardRange = self._v.Metadata, self._v.RewardRange
        self._pending = None
        # The per-instance loop is latency-bound (README.md:32-52): long-lived buffers and their ctypes pointers, so a Step() is one
        # ABI call plus a 4-element copy — no array allocation, no argument marshalling per call.
        v = self._v
        self._discrete = isinstance(self.ActionSpace, Discrete)
        self._a = np.zeros(1, v._adtype)
        self._o = np.empty((1, v.ObsDim), v._dtype)
        self._r = np.empty(1, np.float32)
        self._d = np.empty(1, np.uint8)
        self._pa, self._po, self._pr, self._pd = (x.ctypes.data_as(C.c_void_p) for x in (self._a, self._o, self._r, self._d))
        self._native_step, self._native_reset = v._lib.gymnet_vecenv_step, v._lib.gymnet_vecenv_reset

    def Reset(self):                                                                 # CartPoleEnv.cs:63-67
        st = self._native_reset(self._v._h, self._po)
        if st:
            capi.check(st)
        return self._o[0].copy()                                                     # a COPY, like CartPoleEnv.cs:66

    def Step(self, action):                                                          # CartPoleEnv.cs:137-186
        if isinstance(action, enum.Enum):                                            # Env<TAction> where TAction : Enum (Env.cs:43-53)
            action = int(action.value)
        if self._discrete and (isinstance(action, (bool, np.bool_)) or not isinstance(action, (int, np.integer))):
            raise TypeError(f"Specified cast is not valid: {type(action).__name__} -> int")   # InvalidCastException, :138
        self._a[0] = action
        st = self._native_step(self._v._h, self._pa, self._po, self._pr, self._pd)
        if st:
            capi.check(st)
        d = int(self._d[0])
        # upstream gym's TimeLimit convention for the max_episode_steps extension (done byte, bit 1; the reference has none)
        return Step(self._o[0].copy(), float(self._r[0]), d != 0, {"TimeLimit.truncated": True} if d & 2 else None)

    def StepAsync(self, action):                                                     # Env.cs:23-25, 48-50
        if isinstance(action, enum.Enum):
            action = int(action.value)
        a = np.array([action], dtype=self._v._adtype)
        p = self._v.StepAsync(a)

        class _One:
            def Result(_self):
                return p.Result()[0]
        return _One()

    def Render(self, mode="human"):
        """CartPoleEnv.Render (CartPoleEnv.cs:69-135): "rgb_array" -> uint8 [400, 600, 3] of the current state; "human" -> None (no
        viewer, NullEnvViewer semantics); anything else raises ValueError.  CartPole only (the other envs raise GymNetError)."""
        frames = self._v.Render(mode)
        return None if frames is None else frames[0]

    def CloseEnvironment(self):                                                      # CartPoleEnv.cs:189-194
        self._v.Close()

    Close = Dispose = CloseEnvironment

    def Seed(self, seed):                                                            # CartPoleEnv.cs:196-198
        self._v.Seed(int(seed))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.CloseEnvironment()


class CartPoleEnv(GpuEnv):
    """Drop-in for `new CartPoleEnv()` (README.md:32-52).  Defaults to dtype=float64 — GYMNET_FLAG_F64, the reference's own
    arithmetic (float64 state, the literal CartPoleEnv.cs:141-167 sequence) and its float64 observations (:166,185) — so an
    existing per-instance loop sees the reference's states to the last few ulps and its exact episode lengths, free-running.
    dtype=np.float32 selects the batched engine's float32 arithmetic (1e-5 per teacher-forced step)."""
    ENV = "CartPole-v1"
    DTYPE = np.float64


class PendulumEnv(GpuEnv):
    ENV = "Pendulum-v1"


class MountainCarEnv(GpuEnv):
    ENV = "MountainCar-v0"


class AcrobotEnv(GpuEnv):
    ENV = "Acrobot-v1"


class MountainCarContinuousEnv(GpuEnv):
    """MountainCarContinuous-v0 (upstream gym; absent from the reference): Box(-1, 1, (1,)) force, reward 100 at the goal minus
    0.1 * action^2 of the raw action.  Upstream registers a 999-step time limit: pass max_episode_steps=999 for it (default: none)."""
    ENV = "MountainCarContinuous-v0"


__all__ = ["VectorEnv", "GroupVectorEnv", "DummyVecEnv", "BatchStep", "PendingStep", "GpuEnv", "CartPoleEnv", "PendulumEnv", "MountainCarEnv",
           "AcrobotEnv", "MountainCarContinuousEnv", "AlreadySteppingError", "NotSteppingError"]
