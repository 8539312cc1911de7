// VectorEnv.cs — a VecEnv (src/Gym/Envs/VecEnv.cs:12-93) whose Step/Reset are ONE HIP kernel launch.
// UNVERIFIED: never compiled (no .NET toolchain in the build image).  Drop next to VecEnvWrapper.cs.
//
// Dispatch through the reference's own types.  VecEnv.Seed(int), Seed(int[]) and StepAsync(int) are NOT virtual
// (VecEnv.cs:44-65), so a derived class cannot override them, and `public new` members are invisible to callers that hold
// an IVecEnv or a VecEnv.  Two things make the polymorphic callers work:
//   1. the class RE-LISTS IVecEnv and implements Seed(int) / Seed(int[]) explicitly: every call through IVecEnv
//      (IVecEnv.cs:17-18) lands in the native seed functions;
//   2. `Environments` (VecEnv.cs:25, settable) is a virtual list of N lane proxies.  The non-virtual base Seed — what a
//      VecEnv-typed variable calls — walks Environments and calls Environments[i].Seed(seed[i]) (VecEnv.cs:50-52); each proxy
//      records its lane's seed and the last one flushes the batch to gymnet_vecenv_seed_lanes.  So the base path has the
//      reference's semantics (every env seeded with its own value; Seed(int) = the same value for all, VecEnv.cs:44-46) and
//      its ArgumentException on a length mismatch, without 2^20 IEnv objects ever being stored.
using System;
using System.Collections;
using System.Collections.Generic;
using System.Threading.Tasks;
using Gym.Collections;
using Gym.Observations;
using Gym.Spaces;
using NumSharp;
using SixLabors.ImageSharp;
using SixLabors.ImageSharp.PixelFormats;

namespace Gym.Envs.Amd {
    public sealed unsafe class VectorEnv : VecEnv, IVecEnv, IDisposable {
        private IntPtr _h;
        private GymnetStackFormat _stackFormat;     // of the pixel stack ConfigurePixelStack set up (depth 0: none)
        private int _stackDepth;
        private readonly int _obsDim;
        private readonly bool _boxAction;
        private readonly int _device;
        private readonly bool _f64;                 // GymnetFlags.F64 (CartPole): every observation buffer holds doubles — the reference's
                                                    // actual dtype (CartPoleEnv.cs:166,185); the library writes 8 bytes per element
        internal ulong[] PendingLaneSeeds;          // filled by the lane proxies when the base-class Seed runs
        internal int PendingLaneSeedCount;

        public VectorEnv(GymnetEnvId env, int numEnvs, int device = 0, ulong seed = 0, GymnetFlags flags = GymnetFlags.None,
                         long laneOffset = 0, int maxEpisodeSteps = 0)
            : base(numEnvs, MakeObservationSpace(env, out int obsDim), MakeActionSpace(env, out bool box)) {
            _obsDim = obsDim; _boxAction = box; _device = device;
            _f64 = (flags & GymnetFlags.F64) != 0;
            var cfg = new GymnetConfig {
                struct_size = (uint) sizeof(GymnetConfig), env_id = (int) env, num_envs = numEnvs, lane_offset = laneOffset,
                device = device, flags = (uint) flags, seed = seed, max_episode_steps = maxEpisodeSteps      // (needs GymnetFlags.EpisodeStats)
            };
            Native.Check(Native.gymnet_vecenv_create(ref cfg, out _h));
            Metadata = new Dict("render.modes", new[] {"human", "rgb_array"}, "video.frames_per_second", 50);   // CartPoleEnv.cs:51
            Native.Check(Native.gymnet_env_describe((int) env, out GymnetEnvInfo info));
            RewardRange = (info.reward_low, info.reward_high);
            Environments = new LaneList(this);      // virtual: N proxies materialised on demand, never stored (SURVEY F7)
        }

        internal IntPtr Handle => _h;

        private static Space MakeObservationSpace(GymnetEnvId env, out int obsDim) {
            Native.Check(Native.gymnet_env_describe((int) env, out GymnetEnvInfo i));
            obsDim = i.obs_dim;
            var lo = new float[obsDim]; var hi = new float[obsDim];
            for (int k = 0; k < obsDim; k++) { lo[k] = i.obs_low[k]; hi[k] = i.obs_high[k]; }
            return new Box(np.array(lo), np.array(hi), np.float32);                                               // CartPoleEnv.cs:46-48
        }

        private static Space MakeActionSpace(GymnetEnvId env, out bool box) {
            Native.Check(Native.gymnet_env_describe((int) env, out GymnetEnvInfo i));
            box = i.action_is_box != 0;
            return box ? (Space) new Box(i.action_low, i.action_high, new Shape(1), np.float32) : new Discrete(i.action_n);
        }

        /// An observation buffer of the handle's dtype (float32, or float64 with GymnetFlags.F64), pinned for one native call.
        /// EVERY call that hands the library an `obs_out` goes through here, so the element size can never disagree with the handle.
        private delegate int ObsCall(void* obs);
        private NDArray WithObs(ObsCall call) {
            int n = NumberOfEnvironments;
            if (_f64) {
                var obs = new double[n * _obsDim];
                fixed (double* p = obs) Native.Check(call(p));
                return np.array(obs).reshape(n, _obsDim);
            } else {
                var obs = new float[n * _obsDim];
                fixed (float* p = obs) Native.Check(call(p));
                return np.array(obs).reshape(n, _obsDim);
            }
        }

        /// IVecEnv.Reset() (IVecEnv.cs:14).  Batched form: one NDArray of shape (N, D), float32 — float64 for an F64 handle.
        public NDArray ResetBatch() {
            return WithObs(p => Native.gymnet_vecenv_reset(_h, p));
        }

        public override NDArray[] Reset() {                                                                       // VecEnvWrapper.cs:18-20
            var all = ResetBatch();
            var rows = new NDArray[NumberOfEnvironments];
            for (int i = 0; i < rows.Length; i++) rows[i] = all[i];
            return rows;
        }

        /// The caller's `if (done) Reset()` (README.md:36-40) for the lanes in mask (null = lanes whose last done flag is set).
        public NDArray ResetWhere(byte[] mask = null) {
            if (mask != null && mask.Length != NumberOfEnvironments) throw new ArgumentException("mask length must equal NumberOfEnvironments");
            return WithObs(p => { fixed (byte* m = mask) return Native.gymnet_vecenv_reset_where(_h, m, p); });
        }

        private Step[] ToSteps(NDArray all, float[] rew, byte[] done) {
            var steps = new Step[NumberOfEnvironments];
            for (int i = 0; i < steps.Length; i++) steps[i] = new Step(all[i], rew[i], done[i] != 0, null);       // Step.cs:15-20
            return steps;
        }

        /// IVecEnv.Step(int) (IVecEnv.cs:15): ONE scalar action broadcast to every lane; Step[] materialised per lane.
        public override Step[] Step(int action) {                                                                 // VecEnvWrapper.cs:22-24
            int n = NumberOfEnvironments;
            var rew = new float[n]; var done = new byte[n];
            var obs = WithObs(po => { fixed (float* pr = rew) fixed (byte* pd = done) return Native.gymnet_vecenv_step_broadcast(_h, action, po, pr, pd); });
            return ToSteps(obs, rew, done);
        }

        /// Env<TAction>.Step(TAction) (Env.cs:43-53) for enum-typed discrete actions: the enum's integer value.
        public Step[] Step<TAction>(TAction action) where TAction : Enum => Step((int) (object) action);

        /// EXTENSION: one action per lane (int32 for Discrete, float32 for Box), array-valued results.
        public (NDArray obs, NDArray reward, NDArray done) Step(NDArray actions) {
            int n = NumberOfEnvironments;
            if (actions.size != n) throw new ArgumentException("Number of actions passed should be equals to number of environments");
            var rew = new float[n]; var done = new byte[n];
            var obs = WithObs(po => {
                fixed (float* pr = rew) fixed (byte* pd = done) {
                    if (_boxAction) { var a = actions.astype(np.float32).ToArray<float>(); fixed (float* pa = a) return Native.gymnet_vecenv_step(_h, pa, po, pr, pd); }
                    else { var a = actions.astype(np.int32).ToArray<int>(); fixed (int* pa = a) return Native.gymnet_vecenv_step(_h, pa, po, pr, pd); }
                }
            });
            return (obs, np.array(rew), np.array(done));
        }

        /// ABI 3: the library's page-locked, device-mapped host buffers (valid until Close): actions int32 / float32 [N], obs
        /// float32 [N, D] row-major (float64 for an F64 handle), reward float32 [N], done uint8 [N].  A caller that keeps its NDArrays over this memory
        /// (or reads it through spans) steps with StepPinned(): no managed arrays, no staging copies — the export kernel writes
        /// the results straight across PCIe (0.50 ms per 2^20-lane step instead of 0.57-0.58 ms through pageable arrays).
        public struct PinnedBuffers { public IntPtr Actions; public IntPtr Obs; public IntPtr Reward; public IntPtr Done; }

        public PinnedBuffers HostBuffers() {
            Native.Check(Native.gymnet_vecenv_host_buffers(_h, out IntPtr a, out IntPtr o, out IntPtr r, out IntPtr d));
            return new PinnedBuffers { Actions = a, Obs = o, Reward = r, Done = d };
        }

        /// One vector step over the pinned buffers: reads HostBuffers().Actions, fills Obs / Reward / Done.  Blocks until they are written.
        public void StepPinned() {
            var b = HostBuffers();
            Native.Check(Native.gymnet_vecenv_step(_h, (void*) b.Actions, (void*) b.Obs, (float*) b.Reward, (byte*) b.Done));
        }

        /// ABI 4: override fields of the step kernel's launch configuration (every field of `policy` that is -1 stays as it is;
        /// start from KeepPolicy()).  All configurations compute bit-identical results; a value this handle cannot run throws
        /// ArgumentException.  This is the ONLY way to steer the policy: the library does not read the process environment.
        public static GymnetLaunchPolicy KeepPolicy() => new GymnetLaunchPolicy {
            struct_size = (uint) sizeof(GymnetLaunchPolicy), vec = -1, block = -1, nt = -1, sequential_lanes = -1, reset_form = -1,
            lds_pipe = -1, occupancy_lds_bytes = -1, graph = -1
        };

        public void SetLaunchPolicy(GymnetLaunchPolicy policy) {
            policy.struct_size = (uint) sizeof(GymnetLaunchPolicy);
            Native.Check(Native.gymnet_vecenv_set_launch_policy(_h, ref policy));
        }

        /// ABI 5: `steps` vector steps in ONE kernel launch with what the consumer needs (BasePlaySession.cs:58-69, ReplayMemory.cs:53-67,
        /// TrainingPlaySession.cs:46-52): actions from a device ring, drawn in the kernel (action_source 1: ActionSpace.Sample()) or
        /// epsilon-greedy over the ring (2); dense recording; compact (step, lane, return, length) records of the episodes that end.
        /// All pointers in `spec` are DEVICE pointers; stream-ordered, does not block.
        /// CartPole frames of lanes [firstLane, firstLane + count) (count < 0: to the last lane) into `destination`: a crop of the
        /// 600x400 canvas resized to outW x outH, GRAY8 (1 byte per pixel) or RGB8 (3), lane k's frame at (k - firstLane) * laneStride
        /// bytes (0: frames back to back).  The Images runner's input (CartPoleConfiguration.cs): crop (200, 150, 200, 150) -> 40 x 20,
        /// two frames stacked into 40 x 40 = laneStride 1600 with the second frame written at destination.Slice(800).
        public void RenderFrames(Span<byte> destination, int outW, int outH, int cropX = 0, int cropY = 0, int cropW = 600, int cropH = 400,
                                 long firstLane = 0, long count = -1, long laneStride = 0, GymnetPixelFormat format = GymnetPixelFormat.Gray8) {
            if (count < 0) count = NumberOfEnvironments - firstLane;
            long frame = (long) outW * outH * (format == GymnetPixelFormat.Rgb8 ? 3 : 1);
            if (laneStride == 0) laneStride = frame;
            if (count > 0 && (count - 1) * laneStride + frame > destination.Length)
                throw new ArgumentException("destination is smaller than the frames it must hold", nameof(destination));
            fixed (byte* p = destination)
                Native.Check(Native.gymnet_vecenv_render(_h, p, (int) format, firstLane, count, cropX, cropY, cropW, cropH, outW, outH, laneStride));
        }

        /// CartPoleEnv.Render for one lane: "rgb_array" -> its 600x400 frame, "human" -> null (no viewer window).
        public Image Render(int lane, string mode = "human") {
            if (mode == "human") return null;
            if (mode != "rgb_array") throw new ArgumentException($"unsupported render mode '{mode}'", nameof(mode));
            var rgb = new byte[600 * 400 * 3];
            RenderFrames(rgb, 600, 400, firstLane: lane, count: 1, format: GymnetPixelFormat.Rgb8);
            return Image.LoadPixelData<Rgb24>(rgb, 600, 400);
        }

        /// An episode-aware stack of processed frames per lane on the device (the Images runner's frame queue, ReplayMemory.cs:38-54, and its
        /// input, ImageDataBuilder.cs:10-18): the defaults are two 40 x 20 frames of the crop (200, 150, 200, 150), oldest first, 1.0f where
        /// a pixel is not background.  dExt: a device buffer to adopt (IntPtr.Zero: the handle allocates); laneStride 0: packed
        /// [N][depth][outH][outW].  Replaces any stack the handle had; depth 0 releases it.  CartPole only.
        public void ConfigurePixelStack(GymnetStackFormat format = GymnetStackFormat.BinaryF32, int depth = 2, int outW = 40, int outH = 20,
                                        int cropX = 200, int cropY = 150, int cropW = 200, int cropH = 150, IntPtr dExt = default, long laneStride = 0) {
            Native.Check(Native.gymnet_vecenv_pixel_stack_config(_h, (int) format, depth, cropX, cropY, cropW, cropH, outW, outH, dExt, laneStride));
            _stackFormat = format;
            _stackDepth = depth;
        }

        /// After ResetDevice / a masked reset: the lanes whose device mask byte is set (IntPtr.Zero: every lane) get their current frame in
        /// every slot.
        public void ResetPixelStack(IntPtr dMask = default) => Native.Check(Native.gymnet_vecenv_pixel_stack_reset_device(_h, dMask));

        /// Once per step: lanes whose device done byte is set (IntPtr.Zero: the handle's own done bytes with AutoReset, none without) fill
        /// every slot with the current frame, the others shift by one slot and take it as the newest.
        public void PushPixelStack(IntPtr dDone = default) => Native.Check(Native.gymnet_vecenv_pixel_stack_push_device(_h, dDone));

        /// The stacks of lanes [firstLane, firstLane + count) (count < 0: to the last lane) copied into host memory, packed
        /// [count][depth][outH][outW]: bytes for Gray8 / Binary8 stacks, floats for BinaryF32.  Blocks.
        public void ReadPixelStack(Span<byte> destination, long firstLane = 0, long count = -1) {
            if (_stackFormat == GymnetStackFormat.BinaryF32) throw new ArgumentException("a BinaryF32 stack reads into Span<float>", nameof(destination));
            fixed (byte* p = destination) ReadPixelStack(p, destination.Length, firstLane, count);
        }

        public void ReadPixelStack(Span<float> destination, long firstLane = 0, long count = -1) {
            if (_stackFormat != GymnetStackFormat.BinaryF32) throw new ArgumentException("a byte stack reads into Span<byte>", nameof(destination));
            fixed (float* p = destination) ReadPixelStack(p, (long) destination.Length * 4, firstLane, count);
        }

        private void ReadPixelStack(void* p, long capacityBytes, long firstLane, long count) {
            if (count < 0) count = NumberOfEnvironments - firstLane;
            Native.Check(Native.gymnet_vecenv_pixel_stack_view(_h, out IntPtr dStack, out long laneStride, out long frameBytes));
            if (count > 0 && count * _stackDepth * frameBytes > capacityBytes)
                throw new ArgumentException("destination is smaller than the stacks it must hold", "destination");
            Native.Check(Native.gymnet_vecenv_pixel_stack_read(_h, p, firstLane, count));
        }

        /// The trainer's episode memory on the device (ReplayMemory.Memorize / EndEpisode, MemoryTypes/ReplayMemory.cs:25-67): every step of
        /// each lane's open episode and the best `capacity` finished episodes by (return, end tick, lane), a newer episode winning ties.
        /// maxLength 0 = the handle's max_episode_steps; history = steps per dataset row (MemoryStates).  capacity 0 releases it.
        public void ConfigureEpisodeMemory(int capacity = 100, int maxLength = 0, int history = 4) =>
            Native.Check(Native.gymnet_vecenv_memory_config(_h, capacity, maxLength, history));

        /// ConfigureEpisodeMemory sized for PushMemoryRollout passes of rolloutChunk (1 .. 64) steps: rolloutChunk - 1 more staging slots and
        /// candidate segments.
        public void ConfigureEpisodeMemoryRollout(int capacity = 100, int maxLength = 0, int history = 4, int rolloutChunk = 16) =>
            Native.Check(Native.gymnet_vecenv_memory_config_rollout(_h, capacity, maxLength, history, rolloutChunk));

        /// Once after ONE launch of `steps` steps (any fused rollout, or a single StepDevice with steps = 1): the rows it recorded — dRecObs
        /// [steps][obs_dim][N], dRecReward and dRecDone [steps][N] — and its actions, step t's at row (t % ring) * actionStride of dActions
        /// (a [steps][N] record: actionStride = N, ring = steps).  The memory ends as `steps` x (StepDevice, PushEpisodeMemory) would have left it.
        public void PushMemoryRollout(long steps, IntPtr dRecObs, IntPtr dActions, long actionStride, long ring, IntPtr dRecReward, IntPtr dRecDone) =>
            Native.Check(Native.gymnet_vecenv_memory_push_rollout_device(_h, steps, dRecObs, dActions, actionStride, ring, dRecReward, dRecDone));

        /// Once after each single StepDevice: dActions are the device actions that step took; dDone IntPtr.Zero = the handle's own done bytes.
        public void PushEpisodeMemory(IntPtr dActions, IntPtr dDone = default) =>
            Native.Check(Native.gymnet_vecenv_memory_push_device(_h, dActions, dDone));

        /// After ResetDevice / a masked reset: the masked lanes (IntPtr.Zero: every lane) open a new episode; clearPool also empties the pool.
        public void ResetEpisodeMemory(IntPtr dMask = default, bool clearPool = false) =>
            Native.Check(Native.gymnet_vecenv_memory_reset_device(_h, dMask, clearPool ? 1 : 0));

        /// The kept episodes in descending key order.  Blocks.
        public (float[] Return, int[] Length, ulong[] EndTick, int[] Lane) ReadMemoryEpisodes() {
            Native.Check(Native.gymnet_vecenv_memory_episodes(_h, null, null, null, null, 0, out long count));
            var ret = new float[count]; var len = new int[count]; var tick = new ulong[count]; var lane = new int[count];
            fixed (float* pr = ret) fixed (int* pl = len) fixed (ulong* pt = tick) fixed (int* pn = lane)
                Native.Check(Native.gymnet_vecenv_memory_episodes(_h, pr, pl, pt, pn, count, out count));
            return (ret, len, tick, lane);
        }

        /// DataBuilder.BuildDataset (DataBuilders/DataBuilder.cs:25-55) into device buffers the caller owns, which must hold the rows
        /// DatasetRows() reports: dX float [rows][history * obs_dim] for MemoryParams, else [rows][history][outH][outW] frames (CartPole);
        /// dAction int [rows]; dOneHot float [rows][n] (Discrete only); any may be IntPtr.Zero.  Returns the rows, or -1 while fewer than
        /// minEpisodes episodes are kept (BuildDataset's `return default`).  Ordered on the handle's stream.
        public long BuildMemoryDataset(IntPtr dX, IntPtr dAction, IntPtr dOneHot, long capacityRows, int minEpisodes,
                                       GymnetDatasetFormat format = GymnetDatasetFormat.MemoryParams, int outW = 40, int outH = 20,
                                       int cropX = 200, int cropY = 150, int cropW = 200, int cropH = 150) {
            Native.Check(Native.gymnet_vecenv_memory_stats(_h, out long kept, out _, out _, out _));
            if (kept < minEpisodes) return -1;
            long rows = DatasetRows();
            Native.Check(Native.gymnet_vecenv_memory_dataset_device(_h, (int) format, cropX, cropY, cropW, cropH, outW, outH, dX, dAction, dOneHot,
                                                                    IntPtr.Zero, capacityRows));
            return rows < capacityRows ? rows : capacityRows;
        }

        /// The rows a dataset build writes now.  Blocks.
        public long DatasetRows() {
            Native.Check(Native.gymnet_vecenv_memory_dataset_size(_h, out long rows));
            return rows;
        }

        /// The actor (gymnet_vecenv_actor_config): a fully connected ReLU network on the device that replaces ComposeAction ->
        /// Trainer.Predict -> _network.Forward + IndexOf(Max()) (BasePlaySession.cs:78-81, Trainer.cs:91-92) for every lane, from its last
        /// `history` observations.  widths = w_0 .. w_L (w_0 = history * obs_dim, w_L = action_n); weights = per layer W [out][in] row-major,
        /// then b [out].  NeuralNetworkNET's fully connected weights must be handed over in this [out][in] layout.  No layers releases it.
        public void ConfigureActor(int history, int[] widths, float[] weights) {
            if (widths == null || widths.Length == 0) { Native.Check(Native.gymnet_vecenv_actor_config(_h, 0, 0, null, null, 0)); return; }
            fixed (int* pw = widths) fixed (float* pv = weights)
                Native.Check(Native.gymnet_vecenv_actor_config(_h, history, widths.Length - 1, pw, pv, weights.LongLength));
        }
        /// New device weights of the same widths, ordered on the handle's stream; the history is kept.
        public void LoadActorWeights(IntPtr dWeights, long count) => Native.Check(Native.gymnet_vecenv_actor_load_device(_h, dWeights, count));
        /// After ResetDevice / a masked reset: the masked lanes (IntPtr.Zero: every lane) fill their history with the current observation.
        public void ResetActor(IntPtr dMask = default) => Native.Check(Native.gymnet_vecenv_actor_reset_device(_h, dMask));
        /// Once after each single StepDevice: dDone IntPtr.Zero = the handle's own done bytes.
        public void PushActor(IntPtr dDone = default) => Native.Check(Native.gymnet_vecenv_actor_push_device(_h, dDone));
        /// Every lane's action into dActions (int [N]): argmax of the logits, epsilon-greedy as ComposeActionsDevice would compose it
        /// (TrainingPlaySession.cs:46-52; epsilon 0 = TestingPlaySession); dLogits float [N][action_n] or IntPtr.Zero.
        public void ActorAct(IntPtr dActions, float epsilon = 0f, ulong seed = 0, ulong tick = 0, IntPtr dLogits = default) =>
            Native.Check(Native.gymnet_vecenv_actor_act_device(_h, dActions, dLogits, epsilon, seed, tick));
        /// A Discrete actor's exploration setting (gymnet_vecenv_actor_set_exploration): under Softmax a lane that explores draws its action
        /// from softmax(logits / temperature) instead of uniformly; ActorAct and the fused actor rollout read it.  A new actor has (Uniform, 1).
        public void SetActorExploration(GymnetActorExplore explore, float temperature = 1f) =>
            Native.Check(Native.gymnet_vecenv_actor_set_exploration(_h, (int) explore, temperature));
        public void GetActorExploration(out GymnetActorExplore explore, out float temperature) {
            int ex; float tp;
            Native.Check(Native.gymnet_vecenv_actor_get_exploration(_h, &ex, &tp));
            explore = (GymnetActorExplore) ex; temperature = tp;
        }
        /// ActorAct that also writes the log-probability of every lane's action under softmax(logits / temperature) into dLogp (float [N];
        /// gymnet_vecenv_actor_act_logp_device): the actions and logits are ActorAct's, bit for bit.  IntPtr.Zero: ActorAct itself.
        public void ActorActLogp(IntPtr dActions, IntPtr dLogp, float epsilon = 0f, ulong seed = 0, ulong tick = 0, IntPtr dLogits = default) =>
            Native.Check(Native.gymnet_vecenv_actor_act_logp_device(_h, dActions, dLogits, dLogp, epsilon, seed, tick));
        /// RolloutFused with action_source = actor on a Discrete actor, also recording every step's log-probability into dRecLogp
        /// (float [T][N]; gymnet_vecenv_rollout_fused_logp_device).  IntPtr.Zero: RolloutFused itself.
        public void RolloutFusedLogp(GymnetRolloutSpec spec, IntPtr dRecLogp) {
            spec.struct_size = (uint) sizeof(GymnetRolloutSpec);
            Native.Check(Native.gymnet_vecenv_rollout_fused_logp_device(_h, ref spec, dRecLogp));
        }
        /// The critic (gymnet_vecenv_actor_critic_config): a second network of the actor's kind over the actor's input, widths w_0 =
        /// history * obs_dim .. w_L = 1, whose one output is the lane's value.  Needs a configured actor of either kind; no layers removes
        /// it; ConfigureActor / ConfigureBoxActor drop it.
        public void ConfigureActorCritic(int[] widths, float[] weights) {
            if (widths == null || widths.Length == 0) { Native.Check(Native.gymnet_vecenv_actor_critic_config(_h, 0, null, null, 0)); return; }
            fixed (int* pw = widths) fixed (float* pv = weights)
                Native.Check(Native.gymnet_vecenv_actor_critic_config(_h, widths.Length - 1, pw, pv, weights.LongLength));
        }
        /// New device weights of the critic's widths, ordered on the handle's stream.
        public void LoadActorCriticWeights(IntPtr dWeights, long count) => Native.Check(Native.gymnet_vecenv_actor_critic_load_device(_h, dWeights, count));
        /// The critic over every lane's current history into dValue (float [N]): the last value after a rollout.
        public void ActorValue(IntPtr dValue) => Native.Check(Native.gymnet_vecenv_actor_value_device(_h, dValue));
        /// ActorActLogp that also writes the critic's value of the input each action was chosen from into dValue (float [N];
        /// gymnet_vecenv_actor_act_value_device): actions, logits and logp are ActorActLogp's, bit for bit.  dValue IntPtr.Zero: ActorActLogp itself.
        public void ActorActValue(IntPtr dActions, IntPtr dLogp, IntPtr dValue, float epsilon = 0f, ulong seed = 0, ulong tick = 0, IntPtr dLogits = default) =>
            Native.Check(Native.gymnet_vecenv_actor_act_value_device(_h, dActions, dLogits, dLogp, dValue, epsilon, seed, tick));
        /// RolloutFusedLogp on a Discrete actor with a critic, also recording the value before every step into dRecValue (float [T][N];
        /// gymnet_vecenv_rollout_fused_value_device); dRecLogp may be IntPtr.Zero.  dRecValue IntPtr.Zero: RolloutFusedLogp itself.
        public void RolloutFusedValue(GymnetRolloutSpec spec, IntPtr dRecLogp, IntPtr dRecValue) {
            spec.struct_size = (uint) sizeof(GymnetRolloutSpec);
            Native.Check(Native.gymnet_vecenv_rollout_fused_value_device(_h, ref spec, dRecLogp, dRecValue));
        }
        /// GAE(gamma, lambda) advantages and advantage + value over the rows a rollout recorded (gymnet_gae_device: the recurrence is written
        /// out there), one launch on the handle's device and stream: ordered after the rollout, no synchronise.  dReward float [steps][N],
        /// dDone byte [steps][N] (RolloutFused's records); dValue float [steps][N] or IntPtr.Zero (every value 0), dLastValue float [N],
        /// dBoot float [steps][N] (V(terminal observation) of truncated lanes) or IntPtr.Zero; dAdvantage / dReturn float [steps][N],
        /// either may be IntPtr.Zero.  dAdvantage may be dReward while dReturn is dValue, or the other way round.
        public void AdvantagesDevice(long steps, IntPtr dReward, IntPtr dDone, IntPtr dValue, IntPtr dLastValue, IntPtr dAdvantage, IntPtr dReturn,
                                     float gamma = 0.99f, float lambda = 0.95f, IntPtr dBoot = default) {
            Native.Check(Native.gymnet_vecenv_device_view(_h, out GymnetDeviceView view));
            Native.Check(Native.gymnet_gae_device(_device, view.stream, steps, NumberOfEnvironments, NumberOfEnvironments, dReward, dDone, dValue, dLastValue, dBoot, gamma, lambda, dAdvantage, dReturn));
        }
        /// The actor's history as the caller's own float [history][obs_dim][N], oldest first (gymnet_vecenv_actor_history_device): one kernel
        /// on the handle's stream.  Taken before a fused actor rollout it is the dHistory0 of RolloutInputsDevice.
        public void ActorHistoryDevice(IntPtr dOut) => Native.Check(Native.gymnet_vecenv_actor_history_device(_h, dOut, NumberOfEnvironments));
        /// The network inputs a recorded rollout's actions were chosen from (gymnet_rollout_inputs_device: the rule is written out there), on
        /// the handle's device and stream: ordered after the rollout, no synchronise.  dRecObs [steps][obs_dim][N] in the handle's
        /// observation type, dRecDone byte [steps][N], dHistory0 float [history][obs_dim][N].  dRows IntPtr.Zero: dX is float
        /// [steps][N][history * obs_dim]; else dRows long [numRows] flat indices t * N + lane and dX is [numRows][history * obs_dim].
        /// dHistoryOut (optional) float [history][obs_dim][N]: the history after the last step, the next call's dHistory0.
        public void RolloutInputsDevice(long steps, int history, IntPtr dRecObs, IntPtr dRecDone, IntPtr dHistory0, IntPtr dX,
                                        IntPtr dRows = default, long numRows = 0, IntPtr dHistoryOut = default) {
            Native.Check(Native.gymnet_vecenv_device_view(_h, out GymnetDeviceView view));
            Native.Check(Native.gymnet_rollout_inputs_device(_device, view.stream, steps, NumberOfEnvironments, NumberOfEnvironments, _obsDim, history, _f64 ? 1 : 0, dRecObs, dRecDone, dHistory0, NumberOfEnvironments, dRows, numRows, dX, (long) history * _obsDim, dHistoryOut, NumberOfEnvironments));
        }
        /// The Box actor (gymnet_vecenv_actor_box_config): the same network on Pendulum / MountainCarContinuous with w_L = 1; its one output,
        /// clamped to the env's bounds, is the action.  No layers releases it.  LoadActorWeights / ResetActor / PushActor serve both kinds.
        public void ConfigureBoxActor(int history, int[] widths, float[] weights) {
            if (widths == null || widths.Length == 0) { Native.Check(Native.gymnet_vecenv_actor_box_config(_h, 0, 0, null, null, 0)); return; }
            fixed (int* pw = widths) fixed (float* pv = weights)
                Native.Check(Native.gymnet_vecenv_actor_box_config(_h, history, widths.Length - 1, pw, pv, weights.LongLength));
        }
        /// Every lane's action into dActions (float [N]): the clamped output, or ActionSpace.Sample() where the lane's coin is at or below
        /// epsilon (TrainingPlaySession.cs:46-52 on a Box space); dRaw float [N] or IntPtr.Zero receives the unclamped outputs.
        public void BoxActorAct(IntPtr dActions, float epsilon = 0f, ulong seed = 0, ulong tick = 0, IntPtr dRaw = default) =>
            Native.Check(Native.gymnet_vecenv_actor_box_act_device(_h, dActions, dRaw, epsilon, seed, tick));
        /// A Box actor's policy (gymnet_vecenv_actor_box_set_policy): a tanh head and / or Gaussian noise of scale sigma around the greedy
        /// action on the lanes that explore; BoxActorAct and the fused actor rollout read it.  A new actor has (Clamp, Sample, 0).
        public void SetBoxActorPolicy(GymnetBoxHead head, GymnetBoxExplore explore, float sigma = 0f) =>
            Native.Check(Native.gymnet_vecenv_actor_box_set_policy(_h, (int) head, (int) explore, sigma));
        public void GetBoxActorPolicy(out GymnetBoxHead head, out GymnetBoxExplore explore, out float sigma) {
            int hd, ex; float sg;
            Native.Check(Native.gymnet_vecenv_actor_box_get_policy(_h, &hd, &ex, &sg));
            head = (GymnetBoxHead) hd; explore = (GymnetBoxExplore) ex; sigma = sg;
        }
        /// BoxActorAct that also writes the log-density of every lane's action under the handle's policy, sigma > 0, into dLogd (float [N];
        /// gymnet_vecenv_actor_box_act_logd_device): log N(action; greedy, sigma^2); actions and raw outputs are BoxActorAct's, bit for bit.
        /// IntPtr.Zero: BoxActorAct itself.
        public void BoxActorActLogd(IntPtr dActions, IntPtr dLogd, float epsilon = 0f, ulong seed = 0, ulong tick = 0, IntPtr dRaw = default) =>
            Native.Check(Native.gymnet_vecenv_actor_box_act_logd_device(_h, dActions, dRaw, dLogd, epsilon, seed, tick));
        /// RolloutFused with the actor source on a Box actor, also recording every step's log-density into dRecLogd and, with a critic, the
        /// value before every step into dRecValue (float [T][N] each; gymnet_vecenv_rollout_fused_box_logd_device); either may be
        /// IntPtr.Zero.  Both IntPtr.Zero: RolloutFused itself.
        public void RolloutFusedBoxLogd(GymnetRolloutSpec spec, IntPtr dRecLogd, IntPtr dRecValue) {
            spec.struct_size = (uint) sizeof(GymnetRolloutSpec);
            Native.Check(Native.gymnet_vecenv_rollout_fused_box_logd_device(_h, ref spec, dRecLogd, dRecValue));
        }
        /// V(terminal observation) of every lane whose done byte has bit 1 set (a time limit), +0 for every other lane, into dBoot (float [N]):
        /// one row of AdvantagesDevice's dBoot (gymnet_vecenv_actor_boot_device).  After a vector step and before PushActor; needs a critic
        /// and max_episode_steps > 0, and on an auto-reset handle FinalObs.  Changes neither the history nor what PushActor does next.
        public void ActorBoot(IntPtr dBoot) => Native.Check(Native.gymnet_vecenv_actor_boot_device(_h, dBoot));
        /// RolloutFusedValue / RolloutFusedBoxLogd that also record ActorBoot's row after every step into dRecBoot (float [T][N];
        /// gymnet_vecenv_rollout_fused_value_boot_device, _box_boot_device): needs dRecValue; FinalObs is not needed.  dRecBoot IntPtr.Zero:
        /// the call without it.
        public void RolloutFusedValueBoot(GymnetRolloutSpec spec, IntPtr dRecLogp, IntPtr dRecValue, IntPtr dRecBoot) {
            spec.struct_size = (uint) sizeof(GymnetRolloutSpec);
            Native.Check(Native.gymnet_vecenv_rollout_fused_value_boot_device(_h, ref spec, dRecLogp, dRecValue, dRecBoot));
        }
        public void RolloutFusedBoxBoot(GymnetRolloutSpec spec, IntPtr dRecLogd, IntPtr dRecValue, IntPtr dRecBoot) {
            spec.struct_size = (uint) sizeof(GymnetRolloutSpec);
            Native.Check(Native.gymnet_vecenv_rollout_fused_box_boot_device(_h, ref spec, dRecLogd, dRecValue, dRecBoot));
        }

        public void ResetDevice() => Native.Check(Native.gymnet_vecenv_reset_device(_h));      // device-resident path: nothing crosses PCIe
        public void Sync() => Native.Check(Native.gymnet_vecenv_sync(_h));
        public void RolloutFused(GymnetRolloutSpec spec) {
            spec.struct_size = (uint) sizeof(GymnetRolloutSpec);
            Native.Check(Native.gymnet_vecenv_rollout_fused_ex_device(_h, ref spec));
        }

        /// Frame skip (IGameConfiguration.SkippedFrames, BasePlaySession.cs:37-56): one DECISION, dActions (device, int32 / float32 [N])
        /// held for repeat + 1 env steps inside one launch.  A lane that finishes inside the decision keeps that done byte, is reset
        /// there on an AutoReset handle and idles for the rest; the reward is the sum of the sub-step rewards taken.  repeat in [0, 255].
        public void StepRepeatDevice(IntPtr dActions, int repeat) => Native.Check(Native.gymnet_vecenv_step_repeat_device(_h, dActions, repeat));
        /// The same over the pinned buffers: reads HostBuffers().Actions, fills Obs / Reward / Done.  Blocks until they are written.
        public void StepRepeatPinned(int repeat) {
            var b = HostBuffers();
            Native.Check(Native.gymnet_vecenv_step_repeat(_h, (void*) b.Actions, repeat, (void*) b.Obs, (float*) b.Reward, (byte*) b.Done));
        }
        /// The fused form: spec.steps DECISIONS of repeat + 1 env steps each; the rec_* buffers and the records' step index are per decision.
        public void RolloutRepeat(GymnetRolloutSpec spec, int repeat) {
            spec.struct_size = (uint) sizeof(GymnetRolloutSpec);
            Native.Check(Native.gymnet_vecenv_rollout_repeat_device(_h, ref spec, repeat));
        }

        /// ABI 4: any per-lane array the handle keeps, by id — with GetState / the tick / the seed a complete checkpoint of every
        /// configuration (episode return / length, done flags, per-lane Philox keys, ...).  T must be the array's element type.
        public T[] GetArray<T>(GymnetArrayId which, int count) where T : unmanaged {
            var a = new T[count];
            fixed (T* p = a) Native.Check(Native.gymnet_vecenv_get_array(_h, (int) which, p, (long) count * sizeof(T)));
            return a;
        }

        public void SetArray<T>(GymnetArrayId which, T[] a) where T : unmanaged {
            fixed (T* p = a) Native.Check(Native.gymnet_vecenv_set_array(_h, (int) which, p, (long) a.Length * sizeof(T)));
        }

        /// Compact records of the lanes that finished in the most recent step (GymnetFlags.DoneList [+ EpisodeStats] [+ FinalObs]):
        /// what BasePlaySession.cs:58-69 accumulates per episode, without shipping N flags to the host.
        public (int[] lanes, float[] episodeReturn, int[] episodeLength, float[] finalObs) DoneRecords(bool episode, bool finalObs) {
            int n = NumberOfEnvironments;
            var lanes = new int[n];
            var ret = episode ? new float[n] : null; var len = episode ? new int[n] : null;
            var fo = finalObs ? new float[n * _obsDim] : null;
            long count;
            fixed (int* pl = lanes) fixed (float* pr = ret) fixed (int* pn = len) fixed (float* po = fo)
                Native.Check(Native.gymnet_vecenv_done_records(_h, pl, pr, pn, po, n, out count));
            Array.Resize(ref lanes, (int) count);
            if (episode) { Array.Resize(ref ret, (int) count); Array.Resize(ref len, (int) count); }
            if (finalObs) Array.Resize(ref fo, (int) count * _obsDim);
            return (lanes, ret, len, fo);
        }

        /// VecEnv.StepAsync (VecEnv.cs:63-65) on the native queue: gymnet_vecenv_step_async returns once the step is queued on
        /// the handle's stream; the Task completes in gymnet_vecenv_step_wait.  A second StepAsync before the first finished
        /// surfaces the reference's AlreadySteppingError (AlreadySteppingError.cs:8-10).
        public new Task<Step[]> StepAsync(int action) {
            int n = NumberOfEnvironments;
            if (_boxAction) { var a = new float[n]; for (int i = 0; i < n; i++) a[i] = action; fixed (float* pa = a) Native.Check(Native.gymnet_vecenv_step_async(_h, pa)); }
            else { var a = new int[n]; for (int i = 0; i < n; i++) a[i] = action; fixed (int* pa = a) Native.Check(Native.gymnet_vecenv_step_async(_h, pa)); }
            return Task.Run(() => {
                var rew = new float[n]; var done = new byte[n];
                var obs = WithObs(po => { fixed (float* pr = rew) fixed (byte* pd = done) return Native.gymnet_vecenv_step_wait(_h, po, pr, pd); });
                return ToSteps(obs, rew, done);
            });
        }

        // ---- seeding: explicit IVecEnv implementations (interface callers), `new` members (VectorEnv-typed callers), and the
        //      lane proxies (VecEnv-typed callers, see the header comment)
        void IVecEnv.Seed(int seed) => SeedAll(seed);                                                            // IVecEnv.cs:18
        void IVecEnv.Seed(int[] seed) => SeedLanes(seed);                                                        // IVecEnv.cs:17
        public new void Seed(int seed) => SeedAll(seed);
        public new void Seed(int[] seed) => SeedLanes(seed);

        /// VecEnv.Seed(int) (VecEnv.cs:44-46).  DEVIATION (INTEGRATION.md §0): one Philox key for the batch, lanes differ by counter.
        private void SeedAll(int seed) => Native.Check(Native.gymnet_vecenv_seed(_h, (ulong) seed));

        private void SeedLanes(int[] seed) {                                                                     // VecEnv.cs:48-53
            if (seed == null) throw new ArgumentNullException(nameof(seed));
            var s = Array.ConvertAll(seed, x => (ulong) x);
            Native.Check(Native.gymnet_vecenv_seed_lanes(_h, s, s.Length));     // length mismatch -> ArgumentException (VecEnv.cs:49)
        }

        internal void SeedLaneFromProxy(int lane, int seed) {
            if (PendingLaneSeeds == null) { PendingLaneSeeds = new ulong[NumberOfEnvironments]; PendingLaneSeedCount = 0; }
            PendingLaneSeeds[lane] = (ulong) seed;
            if (++PendingLaneSeedCount == NumberOfEnvironments) {                // the base Seed loop reached the last env
                var s = PendingLaneSeeds; PendingLaneSeeds = null; PendingLaneSeedCount = 0;
                Native.Check(Native.gymnet_vecenv_seed_lanes(_h, s, s.Length));
            }
        }

        public override void Close() {                                                                            // VecEnvWrapper.cs:26-30
            if (_h != IntPtr.Zero) { Native.gymnet_vecenv_destroy(_h); _h = IntPtr.Zero; }
        }

        public void Dispose() => Close();
    }

    /// `Environments` of a VectorEnv: an IList<IEnv> of N lane proxies created on demand (VecEnv.cs:25 lets it be replaced).
    internal sealed class LaneList : IList<IEnv> {
        private readonly VectorEnv _owner;
        public LaneList(VectorEnv owner) { _owner = owner; }
        public int Count => _owner.NumberOfEnvironments;
        public bool IsReadOnly => true;
        public IEnv this[int index] {
            get { if (index < 0 || index >= Count) throw new ArgumentOutOfRangeException(nameof(index)); return new LaneEnv(_owner, index); }
            set => throw new NotSupportedException("the lanes of a VectorEnv are fixed");
        }
        public IEnumerator<IEnv> GetEnumerator() { for (int i = 0; i < Count; i++) yield return new LaneEnv(_owner, i); }
        IEnumerator IEnumerable.GetEnumerator() => GetEnumerator();
        public bool Contains(IEnv item) => item is LaneEnv l && ReferenceEquals(l.Owner, _owner);
        public int IndexOf(IEnv item) => item is LaneEnv l && ReferenceEquals(l.Owner, _owner) ? l.Lane : -1;
        public void CopyTo(IEnv[] array, int arrayIndex) { for (int i = 0; i < Count; i++) array[arrayIndex + i] = new LaneEnv(_owner, i); }
        public void Add(IEnv item) => throw new NotSupportedException();
        public void Clear() => throw new NotSupportedException();
        public void Insert(int index, IEnv item) => throw new NotSupportedException();
        public bool Remove(IEnv item) => throw new NotSupportedException();
        public void RemoveAt(int index) => throw new NotSupportedException();
    }

    /// One lane of a VectorEnv seen as an IEnv (IEnv.cs:11-22).  Seed / Reset act on the lane; a lane cannot be stepped alone.
    internal sealed class LaneEnv : IEnv {
        internal readonly VectorEnv Owner;
        internal readonly int Lane;
        public LaneEnv(VectorEnv owner, int lane) { Owner = owner; Lane = lane; }
        public Dict Metadata { get => Owner.Metadata; set => Owner.Metadata = value; }
        public (float From, float To) RewardRange { get => Owner.RewardRange; set => Owner.RewardRange = value; }
        public Space ActionSpace { get => Owner.ActionSpace; set => Owner.ActionSpace = value; }
        public Space ObservationSpace { get => Owner.ObservationSpace; set => Owner.ObservationSpace = value; }
        public NDArray Reset() { var m = new byte[Owner.NumberOfEnvironments]; m[Lane] = 1; return Owner.ResetWhere(m)[Lane]; }   // CartPoleEnv.cs:63-67
        public Step Step(object action) => throw new NotSupportedException("step the whole batch: VectorEnv.Step(int) / Step(NDArray)");
        public Task<Step> StepAsync(object action) => throw new NotSupportedException("step the whole batch: VectorEnv.StepAsync(int)");
        public Image Render(string mode = "human") => Owner.Render(Lane, mode);   // "rgb_array": the lane's frame; "human": null
        public void CloseEnvironment() { }                                        // the batch owns the resources
        public void Seed(int seed) => Owner.SeedLaneFromProxy(Lane, seed);        // CartPoleEnv.cs:196-198
    }

    /// ONE process driving G GPUs through gymnet_group_* (include/gymnet_amd.h): member m owns lanes [m*N/G, (m+1)*N/G); every
    /// member keeps a replica of all observations, completed by AllGatherObs (hand-written direct push over xGMI, or RCCL).
    public sealed unsafe class GroupVectorEnv : IDisposable {
        private IntPtr _g;
        public int NumberOfEnvironments { get; }
        public int NumMembers { get; }
        public int ObsDim { get; }

        public GroupVectorEnv(GymnetEnvId env, long globalNumEnvs, int[] devices, ulong seed = 0, GymnetFlags flags = GymnetFlags.AutoReset,
                              GymnetGatherMode gather = GymnetGatherMode.Direct) {
            if (devices == null) throw new ArgumentNullException(nameof(devices));
            Native.Check(Native.gymnet_env_describe((int) env, out GymnetEnvInfo info));
            ObsDim = info.obs_dim; NumMembers = devices.Length; NumberOfEnvironments = (int) globalNumEnvs;
            fixed (int* pd = devices) {
                var cfg = new GymnetGroupConfig {
                    struct_size = (uint) sizeof(GymnetGroupConfig), env_id = (int) env, global_num_envs = globalNumEnvs,
                    num_members = devices.Length, flags = (uint) flags, seed = seed, devices = (IntPtr) pd, gather = (int) gather
                };
                Native.Check(Native.gymnet_group_create(ref cfg, out _g));
            }
        }

        public void Seed(int seed) => Native.Check(Native.gymnet_group_seed(_g, (ulong) seed));

        public NDArray Reset() {
            var obs = new float[NumberOfEnvironments * ObsDim];
            fixed (float* p = obs) Native.Check(Native.gymnet_group_reset(_g, p));
            return np.array(obs).reshape(NumberOfEnvironments, ObsDim);
        }

        public (NDArray obs, NDArray reward, NDArray done) Step(int[] actions) {
            int n = NumberOfEnvironments;
            if (actions.Length != n) throw new ArgumentException("Number of actions passed should be equals to number of environments");
            var obs = new float[n * ObsDim]; var rew = new float[n]; var done = new byte[n];
            fixed (int* pa = actions) fixed (float* po = obs) fixed (float* pr = rew) fixed (byte* pd = done)
                Native.Check(Native.gymnet_group_step(_g, pa, po, pr, pd));
            return (np.array(obs).reshape(n, ObsDim), np.array(rew), np.array(done));
        }

        public void StepDevice(IntPtr[] dActions) => Native.Check(Native.gymnet_group_step_device(_g, dActions));
        public void AllGatherObs() => Native.Check(Native.gymnet_group_allgather_obs(_g));
        public void WaitGather() => Native.Check(Native.gymnet_group_wait_gather(_g));
        public IntPtr GlobalObs(int member) { Native.Check(Native.gymnet_group_global_obs(_g, member, out IntPtr p)); return p; }
        public void Sync() => Native.Check(Native.gymnet_group_sync(_g));

        public void Dispose() { if (_g != IntPtr.Zero) { Native.gymnet_group_destroy(_g); _g = IntPtr.Zero; } }
    }
}
