"""The attachments (actor with its critic / logp / logd / boot units, pixel stack, episode memory) and the fused actor rollout on every
handle layout that changes where "the current observation" lives or which Philox key a lane draws with:

  DB            double_buffer=True: the observation buffer changes identity after every step and after every fused launch
  EXT           caller-owned observation buffer with a padded stride (n + 12 elements), sentinel in the pad columns and past the last row
  EXT+DB        two caller-owned buffers, double buffered
  KEYS          per-lane Philox keys (three distinct ones) installed after Reset and followed by a Reset
  OFF           lane_offset = 2^32 + 5
  LIST / LIST_COMPACT   done_list + final_obs, without and with compact_records_only

at 259 lanes (four waves and three lanes), T = 12, max_episode_steps = 5 where a limit exists.  Everything is bit for bit: two device
paths on uint32 / uint8 views, a twin through twin.same (-0 == +0).  No tolerance anywhere.  Where a layout has caller-owned buffers, every
pad column and everything past the last row must still hold the sentinel afterwards, and the library's DeviceView must point into them."""
import numpy as np
import pytest

import _actor_boot_cases as cases
import _actor_forms as forms
import _actor_logp_twin as logp_twin
import _actor_twin as twin
import _episode_memory_model as mem_model
import _pixel_stack_model as stack_model

pytestmark = pytest.mark.gpu
SEED = 0xAC7
F32 = np.float32
N, T, S, LIMIT, PAD, TAIL = 259, 12, 2, 5, 12, 64
SENTINEL = -12345.5
CARTPOLE, MOUNTAINCAR, ACROBOT, PENDULUM, MCC = "CartPole-v1", "MountainCar-v0", "Acrobot-v1", "Pendulum-v1", "MountainCarContinuous-v0"
OBS, ACTIONS = cases.OBS, {CARTPOLE: 2, MOUNTAINCAR: 3, ACROBOT: 3}
BOX_ENVS = (PENDULUM, MCC)
ALIAS = (CARTPOLE, MOUNTAINCAR, MCC)                 # envs whose observation IS their state: the caller's buffer is the state buffer
POISON = 7.25


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def u32(a):
    a = np.ascontiguousarray(a if isinstance(a, np.ndarray) else host(a))
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


class Layout:
    """One layout: kwargs(k) are handle k's own VectorEnv arguments, prepare(env) runs after the first Reset (paints the sentinel into
    the caller's buffers, installs the keys), after(env) checks the sentinel and the DeviceView."""

    def __init__(self, kind, env_name, n=N, dtype=np.float32):
        self.kind, self.env_name, self.n, self.dtype = kind, env_name, n, np.dtype(dtype)
        self.rows = OBS[env_name]
        self.stride = n + PAD
        self.bufs = []                          # per handle: the tensors it was given

    @property
    def ext(self):
        return self.kind in ("EXT", "EXT+DB")

    def shared(self):
        kw = {}
        if self.kind in ("DB", "EXT+DB"):
            kw["double_buffer"] = True
        if self.kind == "OFF":
            kw["lane_offset"] = 2 ** 32 + 5
        if self.kind in ("LIST", "LIST_COMPACT"):
            kw.update(done_list=True, final_obs=True)
        if self.kind == "LIST_COMPACT":
            kw["compact_records_only"] = True
        if self.dtype == np.float64:
            kw["dtype"] = np.float64
        return kw

    def kwargs(self, k=0):
        if not self.ext:
            return {}
        import torch
        count = 2 if self.kind == "EXT+DB" else 1
        bufs = [torch.zeros(self.rows * self.stride + TAIL, dtype=getattr(torch, self.dtype.name), device="cuda") for _ in range(count)]
        torch.cuda.synchronize()
        assert all(b.data_ptr() % 16 == 0 for b in bufs)
        self.bufs.append(bufs)
        kw = dict(ext_obs=bufs[0], ext_obs_stride=self.stride)
        if count == 2:
            kw["ext_obs_alt"] = bufs[1]
        return kw

    def per_handle(self, k):
        return dict(kwargs=self.kwargs(k), after=self.after)

    def _mine(self, env):
        """the buffers this handle was given, found through the library's own view of where its observations live"""
        v = env.DeviceView()
        for bufs in self.bufs:
            ptrs = [b.data_ptr() for b in bufs]
            if v.d_obs in ptrs:
                assert v.obs_stride == self.stride
                if len(bufs) == 2:
                    assert v.d_obs_alt in ptrs and v.d_obs_alt != v.d_obs
                if self.env_name in ALIAS:
                    assert v.d_state == v.d_obs and v.state_stride == self.stride
                return bufs
        raise AssertionError("the handle's observation view points into none of the caller's buffers")

    def _pads(self, buf):
        body = buf[:self.rows * self.stride].view(self.rows, self.stride)
        return body[:, self.n:], buf[self.rows * self.stride:]

    def prepare(self, env):
        import torch
        if self.ext:
            env.Sync()                          # (create zeroes through the pad columns of all rows but the last: paint afterwards)
            for buf in self._mine(env):
                for part in self._pads(buf):
                    part.fill_(SENTINEL)
            torch.cuda.synchronize()
        if self.kind == "KEYS":
            keys = 0x1234_0000_0000 + np.arange(self.n) % 3
            assert len(set(keys.tolist())) == 3
            env.Seed(keys)
            env.Reset()
            assert env.GetSeed()[1]

    def after(self, env):
        if not self.ext:
            return
        env.Sync()
        for buf in self._mine(env):
            for part in self._pads(buf):
                assert (host(part) == SENTINEL).all(), "a pad column or the tail past the last row was written"


def _goal(name):
    def place(env):
        if name in cases.GOAL_ENVS:
            env.SetState(cases.at_the_goal(name, env.GetState()))
    return place


def _discrete_net(name, seed=1):
    return twin.net(np.random.default_rng([seed, OBS[name]]), [S * OBS[name], 16, ACTIONS[name]], scale=2.0)


def _box_net(name, seed=2):
    return twin.net(np.random.default_rng([seed, OBS[name]]), [S * OBS[name], 16, 1], scale=2.0)


# ---- 1. the Discrete actor's fused rollout against T x actor.Step: lean, bookkeeping and records forms, both exploration settings --------
def _discrete_cases():
    out = []
    # (LIST_COMPACT is in the second test alone: this comparison reads the dense finished-episode views after the whole rollout, and a
    # compact-records-only handle defines them for the steps the caller read, which the single-step handle did and the fused one cannot)
    for name, kinds in ((CARTPOLE, ("DB", "EXT", "EXT+DB", "KEYS", "OFF", "LIST")), (ACROBOT, ("DB", "EXT+DB", "KEYS")),
                        (MOUNTAINCAR, ("DB", "EXT+DB", "KEYS"))):
        for kind in kinds:
            lists = kind.startswith("LIST")
            for shape, auto in (("lean", True), ("book", True), ("records", True), ("book", False)):
                if lists and (shape == "lean" or not auto):
                    continue                    # final_obs needs auto_reset; the done records compared need the bookkeeping
                for setting in (("uniform", 1.0), ("softmax", 0.5)):
                    out.append(pytest.param(name, kind, shape, auto, setting, id=f"{name}-{kind}-{shape}-{'auto' if auto else 'noreset'}-{setting[0]}"))
    return out


@pytest.mark.parametrize("name,kind,shape,auto,setting", _discrete_cases())
def test_discrete_fused_rollout_equals_single_steps(gpu_pkg, name, kind, shape, auto, setting):
    lay = Layout(kind, name)
    kw = dict(auto_reset=auto, **lay.shared())
    if shape != "lean":
        kw.update(episode_stats=True, max_episode_steps=LIMIT)
    place = _goal(name)

    def prepare(env):
        lay.prepare(env)
        place(env)
    out = forms.fused_equals_single_steps(gpu_pkg, name, N, T, kw, shape == "records", _discrete_net(name)[2], S=S, eps=0.5,
                                          full=kind.startswith("LIST"), prepare=prepare, per_handle=lay.per_handle,
                                          configure=lambda env, actor: actor.SetExploration(*setting))
    assert len(np.unique(out["actions"])) == ACTIONS[name]
    if shape != "lean":
        assert (out["done"] & 2).any()                                       # the time limit strikes
        if auto:
            assert ((out["done"] & 2) != 0).sum(axis=0).max() >= 2            # a lane truncates, restarts and truncates again
    if name != CARTPOLE:
        assert (out["done"][0] & 1).any()                                    # and the goal lanes terminate in the first step
    if lay.ext:
        assert len(lay.bufs) == 2


# ---- 2. the recording units: Act(logits, logp, value) / Value / Boot against their twins at every step, and the fused rollout with
#         rec_logp / rec_logd, rec_value and rec_boot against those steps -----------------------------------------------------------------
def _unit_cases():
    out = []
    for name, kinds in ((CARTPOLE, ("DB", "EXT", "EXT+DB", "KEYS", "OFF", "LIST", "LIST_COMPACT")), (ACROBOT, ("DB", "EXT+DB", "KEYS")),
                        (MOUNTAINCAR, ("DB", "EXT+DB", "KEYS"))):
        for kind in kinds:
            for setting in (("uniform", 1.0), ("softmax", 0.5)):
                out.append(pytest.param(name, kind, setting, id=f"{name}-{kind}-{setting[0]}"))
    for name in BOX_ENVS:
        for kind in ("DB", "EXT+DB", "KEYS", "OFF"):
            for policy in (("clamp", "sample", 0.0), ("tanh", "gaussian", 0.3)):
                out.append(pytest.param(name, kind, policy, id=f"{name}-{kind}-{policy[0]}-{policy[1]}"))
    return out


@pytest.mark.parametrize("name,kind,setting", _unit_cases())
def test_recording_units_equal_their_twins_and_the_fused_rollout(gpu_pkg, name, kind, setting):
    """Handle a: T x (Act with every output, StepDevice, Boot, Push), every output against its twin over History(); handle b: one fused
    rollout that records the same streams.  A Box actor under the default policy has no log-density (sigma = 0) and, through this API,
    no recorded value: its rollout records actions only.  LIST_COMPACT: the dense terminal observations are not maintained, so the
    stand-alone Boot is refused (nothing written) while the fused rollout's rec_boot, which needs no final_obs, is compared with the twin."""
    import torch
    box = name in BOX_ENVS
    lay = Layout(kind, name)
    eps, seed, tick0 = 0.5, 99, 1000
    kw = dict(auto_reset=True, episode_stats=True, max_episode_steps=LIMIT, **lay.shared())
    kw["final_obs"] = True
    w, flat, pairs = (_box_net if box else _discrete_net)(name)
    critic = cases.critic(name, False)
    recorded = not box or setting[2] > 0                                   # lp / value / boot are recorded
    boot_alone = kind != "LIST_COMPACT"
    temperature = 1.0 if box else setting[1]
    envs = [gpu_pkg.VectorEnv(name, N, seed=SEED, **kw, **lay.kwargs(k)) for k in (0, 1)]
    try:
        actors = []
        for env in envs:
            env.Reset()
            lay.prepare(env)
            actor = env.Actor(pairs, history=S)
            actor.SetCritic(critic[2])
            for t in range(3):
                actor.Step(eps, seed + 1, t)
            _goal(name)(env)
            env.SetArray("episode_length", (np.arange(N) % LIMIT).astype(np.int32))     # staggered: some lanes truncate in every step
            actor.Reset()
            if box:
                actor.SetPolicy(*setting)
            else:
                actor.SetExploration(*setting)
            actors.append(actor)
        (a, b), (actor_a, actor_b) = envs, actors
        tick_start, O = a.Tick, a.ObsDim
        acts = torch.empty(N, dtype=torch.float32 if box else torch.int32, device="cuda")
        lg = torch.empty((N, 1 if box else ACTIONS[name]), dtype=torch.float32, device="cuda")
        lp, vl, bt = (torch.full((N,), POISON, dtype=torch.float32, device="cuda") for _ in range(3))
        torch.cuda.synchronize()
        rows = dict(act=[], obs=[], rew=[], done=[], lp=[], value=[], boot=[], want_boot=[], fin=[])
        for t in range(T):
            hist = actor_a.History()
            x = np.ascontiguousarray(hist.reshape(N, -1))
            want_value = twin.forward(critic[0], critic[1], x)[0][:, 0]
            if box:
                actor_a.Value(out=vl)
                actor_a.Act(eps, seed, tick0 + t, out=acts, logits=lg, logd=lp if recorded else None)
            else:
                actor_a.Act(eps, seed, tick0 + t, out=acts, logits=lg, logp=lp, value=vl)
            got_act = host(acts).copy()
            assert twin.same(host(lg), twin.forward(w, flat, x)[0]), t        # the network's outputs over the history
            assert twin.same(host(vl), want_value), t
            if not box:
                assert np.array_equal(u32(lp), logp_twin.logp(host(lg), got_act, temperature)), t
            a.StepDevice(acts)
            done = a.GetArray("done")
            want_boot = cases.want_boot(critic, hist, a.GetArray("final_obs").T, done)   # (the getter applies compact records on demand)
            if boot_alone:
                actor_a.Boot(out=bt)
                assert twin.same(host(bt), want_boot), t
            else:
                with pytest.raises(ValueError, match="COMPACT_RECORDS_ONLY"):
                    actor_a.Boot(out=bt)
                assert (host(bt) == F32(POISON)).all()                        # the refusal wrote nothing
            rows["want_boot"].append(want_boot)
            rows["fin"].append((a.GetArray("finished_return"), a.GetArray("finished_length")))
            actor_a.Push()
            r = a.Read()
            rows["act"].append(got_act); rows["obs"].append(r.Observation.T.copy()); rows["rew"].append(r.Reward.copy()); rows["done"].append(done)
            rows["lp"].append(u32(lp).copy()); rows["value"].append(u32(vl).copy()); rows["boot"].append(u32(bt).copy())
        done_a = np.stack(rows["done"])
        assert (done_a & 2).any() and ((done_a & 2) != 0).sum(axis=0).max() >= 2
        if name in cases.GOAL_ENVS:
            assert (done_a & 1).any()
        rec = dict(rec_obs=torch.empty((T, O, N), dtype=torch.float32, device="cuda"), rec_reward=torch.empty((T, N), dtype=torch.float32, device="cuda"),
                   rec_done=torch.empty((T, N), dtype=torch.uint8, device="cuda"),
                   rec_actions=torch.empty((T, N), dtype=torch.float32 if box else torch.int32, device="cuda"))
        lp_b, val_b, boot_b = (torch.full((T + 1, N), POISON, dtype=torch.float32, device="cuda") for _ in range(3))
        torch.cuda.synchronize()
        ep = forms.episode_buffers(T * N)
        more = dict(episodes=ep)
        if recorded:
            more.update(rec_value=val_b[:T], rec_boot=boot_b[:T], **({"rec_logd": lp_b[:T]} if box else {"rec_logp": lp_b[:T]}))
        b.RolloutFusedDevice(None, T, actions="actor", epsilon=eps, action_seed=seed, action_tick0=tick0, **rec, **more)
        assert np.array_equal(u32(rec["rec_actions"]), u32(np.stack(rows["act"])))
        assert np.array_equal(u32(rec["rec_obs"]), u32(np.stack(rows["obs"]).astype(F32)))
        assert np.array_equal(u32(rec["rec_reward"]), u32(np.stack(rows["rew"])))
        assert np.array_equal(host(rec["rec_done"]), done_a)
        want = sorted((t, int(lane), float(rows["fin"][t][0][lane]), int(rows["fin"][t][1][lane])) for t in range(T) for lane in np.nonzero(done_a[t])[0])
        got, kept, ended = forms.records(ep)
        assert ended == kept == len(want) and got == want                    # the episode records: step, lane, return and length
        if kind.startswith("LIST"):                                          # the last step's done list and compact records
            ra, rb = a.DoneRecords(), b.DoneRecords()
            ka, kb = np.argsort(ra["lanes"]), np.argsort(rb["lanes"])
            assert np.array_equal(ra["lanes"][ka], np.nonzero(done_a[-1])[0])
            for k in ("lanes", "return", "length", "final_obs"):
                assert np.array_equal(u32(ra[k][ka]), u32(rb[k][kb])), k
        if recorded:
            assert np.array_equal(u32(lp_b)[:T], np.stack(rows["lp"]))
            assert np.array_equal(u32(val_b)[:T], np.stack(rows["value"]))
            if boot_alone:
                assert np.array_equal(u32(boot_b)[:T], np.stack(rows["boot"]))
            assert twin.same(host(boot_b)[:T], np.stack(rows["want_boot"]))  # the definition (the rollout's boot needs no dense final_obs)
            assert (u32(boot_b)[:T][(done_a & 2) == 0] == 0).all()          # +0.0f where no time limit struck
            for buf in (lp_b, val_b, boot_b):
                assert (host(buf)[T] == F32(POISON)).all()                   # nothing past row T - 1
        else:
            for buf in (lp_b, val_b, boot_b):
                assert (host(buf) == F32(POISON)).all()
        assert np.array_equal(u32(a.GetState()), u32(b.GetState())) and np.array_equal(a.GetArray("done"), b.GetArray("done"))
        assert a.Tick == b.Tick == tick_start + T
        # (compact records only: the dense rows are brought up to date for the lanes of the most recent step, and a's getters ran every step)
        last = done_a[-1] != 0 if kind == "LIST_COMPACT" else np.ones(N, bool)
        for k in ("episode_return", "episode_length"):
            assert np.array_equal(u32(a.GetArray(k)), u32(b.GetArray(k))), k
        for k in ("finished_return", "finished_length", "final_obs"):
            assert np.array_equal(u32(a.GetArray(k))[..., last], u32(b.GetArray(k))[..., last]), k
        assert np.array_equal(actor_a.History(), actor_b.History())
        assert np.array_equal(u32(actor_a.Value()), u32(actor_b.Value()))
        assert np.array_equal(u32(actor_a.Step(eps, seed, tick0 + T)), u32(actor_b.Step(eps, seed, tick0 + T)))
        for env in envs:
            lay.after(env)
    finally:
        for env in envs:
            env.Close()


# ---- 3. the pixel stack ------------------------------------------------------------------------------------------------------------
def _gray(env, crop, size):
    import torch
    out = torch.empty((env.NumberOfEnvironments, size[1], size[0]), dtype=torch.uint8, device="cuda")
    env.RenderDevice(out, "gray", crop=crop, size=size)
    env.Sync()
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["DB", "EXT", "EXT+DB"])
def test_pixel_stack_slots_equal_the_render_of_the_current_observation(gpu_pkg, kind, dtype):
    """20 pushes with restarts.  After every push each slot equals what RenderDevice draws from the handle at that moment, combined by the
    stack model's rules — and that render equals the one of a plain handle (one library-owned buffer) that took the same actions, so a
    stack and a render that both looked at the buffer of the step before would not pass."""
    crop, size, depth = (200, 150, 200, 150), (40, 20), 3
    lay = Layout(kind, CARTPOLE, dtype=dtype)
    rng = np.random.default_rng(7)
    kw = dict(seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=LIMIT)
    with gpu_pkg.VectorEnv(CARTPOLE, N, **kw, **lay.shared(), **lay.kwargs()) as env, \
            gpu_pkg.VectorEnv(CARTPOLE, N, dtype=dtype, **kw) as ref:
        env.Reset(); ref.Reset()
        lay.prepare(env)
        for e in (env, ref):                                                  # staggered time limits: some lanes restart in every push
            e.SetArray("episode_length", (np.arange(N) % LIMIT).astype(np.int32))
        st = env.PixelStack(depth=depth, size=size, crop=crop, format="gray8")
        m = stack_model.PixelStackModel(_gray(env, crop, size), depth)
        assert np.array_equal(st.Read(), m.stack)
        restarts = appended = mixed = 0
        for t in range(20):
            a = dev(rng.integers(0, 2, N).astype(np.int32))
            st.Step(a)
            ref.StepDevice(a)
            g = _gray(env, crop, size)
            assert np.array_equal(g, _gray(ref, crop, size)), t
            done = env.GetArray("done")
            assert np.array_equal(done, ref.GetArray("done")) and np.array_equal(u32(env.GetState()), u32(ref.GetState()))
            assert np.array_equal(st.Read(), m.push(g, done)), t
            if t == 9:                                                        # a masked reset of handle and stack in between
                mask = (np.arange(N) % 4 == 1).astype(np.uint8)
                d_mask = dev(mask)
                env.ResetWhereDevice(d_mask); ref.ResetWhereDevice(d_mask)
                st.Reset(d_mask)
                assert np.array_equal(st.Read(), m.reset(_gray(env, crop, size), mask))
            restarts += int((done != 0).sum()); appended += int((done == 0).sum())
            mixed += int((done != 0).any() and (done == 0).any())
        assert mixed == 20 and restarts > N and appended > N                  # every push restarts some lanes while others append
        lay.after(env)


# ---- 4. the episode memory -----------------------------------------------------------------------------------------------------------
def _mem_actions(env, rng, t):
    n = env.NumberOfEnvironments
    if env._adtype == np.float32:
        return rng.uniform(env._info.action_low, env._info.action_high, n).astype(np.float32)
    return mem_model.mixed_policy(n, rng, t, env.ActionSpace.N)


def _mem_snapshot(mem):
    data = mem.BuildDataset("params", min_episodes=0, reward=True) if mem.DatasetSize() else None
    return dict(stats=mem.Stats(), episodes=mem.Episodes(), data=None if data is None else [None if v is None else host(v) for v in data])


def _mem_same(x, y):
    assert x["stats"] == y["stats"]
    for g, w in zip(x["episodes"], y["episodes"]):
        assert np.array_equal(g, w)
    assert (x["data"] is None) == (y["data"] is None)
    for g, w in zip(x["data"] or [], y["data"] or []):
        assert (g is None) == (w is None)
        if g is not None:
            assert g.shape == w.shape and np.array_equal(u32(g), u32(w))


@pytest.mark.parametrize("name,dtype", [(CARTPOLE, np.float32), (CARTPOLE, np.float64), (PENDULUM, np.float32)], ids=["cartpole", "cartpole-f64", "pendulum"])
@pytest.mark.parametrize("kind", ["DB", "EXT+DB", "KEYS", "OFF"])
def test_episode_memory_equals_the_model_and_the_ingest_equals_single_pushes(gpu_pkg, kind, name, dtype):
    """Handle a: mem.Step x T against the NumPy model fed with what the step API returned (kept set and counters after every push, the
    params dataset at the end).  Handle b: mem.Rollout(T) with rollout_chunk = 4 over the same actions: stats, Episodes() and the params
    dataset are a's, bit for bit."""
    capacity, history = 6, 2
    lays = [Layout(kind, name, dtype=dtype), Layout(kind, name, dtype=dtype)]
    rng = np.random.default_rng(11)
    kw = dict(seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=LIMIT)
    with gpu_pkg.VectorEnv(name, N, **kw, **lays[0].shared(), **lays[0].kwargs()) as a, \
            gpu_pkg.VectorEnv(name, N, **kw, **lays[1].shared(), **lays[1].kwargs()) as b:
        for env, lay in zip((a, b), lays):
            env.Reset()
            lay.prepare(env)
            env.SetArray("episode_length", (np.arange(N) % LIMIT).astype(np.int32))
        obs0 = a.Read().Observation
        mem_a = a.EpisodeMemory(capacity=capacity, max_length=0, history=history)
        mem_b = b.EpisodeMemory(capacity=capacity, max_length=0, history=history, rollout_chunk=4)
        m = mem_model.EpisodeMemoryModel(obs0, capacity, LIMIT, history)
        stride = (N + 63) // 64 * 64
        acts = np.stack([_mem_actions(a, rng, t) for t in range(T)])
        ring = dev(np.pad(acts, ((0, 0), (0, stride - N))))
        dones = []
        for t in range(T):
            mem_a.Step(ring[t])
            out = a.Read()
            d = a.GetArray("done")
            m.push(acts[t], out.Reward, d, out.Observation, a.Tick)
            got, want = mem_a.Episodes(), m.kept()
            for g, w_, what in zip(got, want, ("return", "length", "end_tick", "lane")):
                assert np.array_equal(g, w_), (t, what)
            s = mem_a.Stats()
            assert (s["kept"], s["ended"], s["too_long"], s["admitted"]) == (len(m.pool), m.ended, m.too_long, m.admitted), t
            dones.append(d)
        dones = np.stack(dones)
        assert (dones != 0).any(axis=1).all() and (dones == 0).any(axis=1).all()          # every push restarts some lanes and appends to others
        assert (dones & 2).any() and m.ended > capacity
        snap_a = _mem_snapshot(mem_a)
        x, act, onehot, rew = m.dataset_params(None if a._adtype == np.float32 else a.ActionSpace.N)
        assert snap_a["data"] is not None and len(x) > 0
        gx, gact, gone, grew = snap_a["data"]
        assert np.array_equal(u32(gx), u32(x)) and np.array_equal(u32(gact), u32(act.astype(gact.dtype))) and np.array_equal(u32(grew), u32(rew))
        if onehot is not None:
            assert np.array_equal(u32(gone), u32(onehot))
        taken = mem_b.Rollout(T, ring, action_stride=stride, ring=T)
        assert taken is ring
        _mem_same(_mem_snapshot(mem_b), snap_a)
        assert np.array_equal(u32(a.GetState()), u32(b.GetState())) and a.Tick == b.Tick
        for env, lay in zip((a, b), lays):
            lay.after(env)
