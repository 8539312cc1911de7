"""GPU tests of frame skip (gym.net_amd/csrc/action_repeat.hip; gymnet_vecenv_step_repeat_device / _step_repeat / _rollout_repeat_device):
an action held for R = repeat + 1 env steps inside one launch.  Every comparison is bitwise.

  * repeat = 0 is the one-step call: six env / dtype combinations x {auto-reset, not} x {lean, bookkeeping} at 130 lanes against a twin
    handle's StepDevice, and RolloutFusedDevice(repeat=0) against the same call without the argument;
  * one decision against the NumPy model (tests/_action_repeat_model.py), R = 2, 4, 8 at 1, 63, 65, 257 and 1000 lanes, 40 decisions.  The
    test ASSERTS FROM THE MODEL that the freeze path is exercised: for every sub-step r at least one lane finished at r (wherever the
    batch has a lane per sub-step index: one lane under one time limit can only ever finish at one index), and for CartPole that at
    least a quarter of the lanes finished at all;
  * DOUBLE_BUFFER, a non-zero lane_offset (2048 lanes = 1000 + 1048 on two handles) and engine tick 2^32 - 3 with R = 4;
  * the fused form equals single decisions on a twin handle, for every row of tests/_action_repeat_forms.py at 1000 lanes, T = 12;
  * the attachments at the Images runner's R = 2 (CartPole, 257 lanes, max_episode_steps 9): pixel stack, episode memory and actor against
    their models / an unfused twin, and the pushes that stay refused;
  * refusals, and the host boundary."""
import ctypes as C

import numpy as np
import pytest

import _action_repeat_forms as forms
import _action_repeat_model as model
import _actor_twin as actor_twin
import _episode_memory_model as memory_model
import _pixel_stack_model as stack_model

pytestmark = pytest.mark.gpu
SEED, ASEED = 0x5EED, 0xAC710
F32 = np.float32
NAMES = list(forms.ENVS)


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _make(gpu_pkg, name, n, **kw):
    gym, dt = forms.ENVS[name]
    return gpu_pkg.VectorEnv(gym, n, dtype=dt, **kw)


def _random_actions(name, rng, n):
    _, _, box, nact = model.ENVS[name]
    if box:
        lo, hi = (-2.0, 2.0) if name == "Pendulum" else (-1.0, 1.0)
        return rng.uniform(lo, hi, n).astype(F32)
    return rng.integers(0, nact, n).astype(np.int32)


# ---- repeat = 0 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("auto", [True, False])
@pytest.mark.parametrize("book", [False, True])
def test_repeat_0_is_the_one_step_call(gpu_pkg, name, auto, book):
    n = 130
    rng = np.random.default_rng(5)
    kw = dict(seed=SEED, auto_reset=auto)
    if book:
        kw.update(episode_stats=True, max_episode_steps=7)
    with _make(gpu_pkg, name, n, **kw) as f, _make(gpu_pkg, name, n, **kw) as e:
        f.Reset(); e.Reset()
        for t in range(12):
            a = _dev(_random_actions(name, rng, n))
            f.StepRepeatDevice(a, 0)
            e.StepDevice(a)
            x, y = f.Read(), e.Read()
            assert np.array_equal(f.GetState(), e.GetState()) and f.Tick == e.Tick, t
            assert np.array_equal(x.Observation, y.Observation) and np.array_equal(x.Reward.view(np.uint32), y.Reward.view(np.uint32)), t
            assert np.array_equal(f.GetArray("done"), e.GetArray("done")), t
            if name.startswith("CartPole") and not auto:
                assert np.array_equal(f.GetStepsBeyondDone(), e.GetStepsBeyondDone()), t
                assert f.Counters()["stepped_after_done"] == e.Counters()["stepped_after_done"]
            if book:
                for arr in ("episode_return", "episode_length", "finished_return", "finished_length"):
                    assert np.array_equal(f.GetArray(arr), e.GetArray(arr)), (arr, t)
        host = _random_actions(name, rng, n)
        x, y = f.StepRepeat(host, 0), e.Step(host)
        assert np.array_equal(x.Observation, y.Observation) and np.array_equal(x.Reward, y.Reward) and np.array_equal(x.Done, y.Done)
        ring = _dev(np.stack([_random_actions(name, rng, n) for _ in range(2)]))
        f.RolloutFusedDevice(ring, 5, n, 2, repeat=0)
        e.RolloutFusedDevice(ring, 5, n, 2)
        assert np.array_equal(f.GetState(), e.GetState()) and f.Tick == e.Tick
        assert np.array_equal(f.GetArray("reward"), e.GetArray("reward")) and np.array_equal(f.GetArray("done"), e.GetArray("done"))
        assert f.Counters()["lane_steps"] == e.Counters()["lane_steps"]


# ---- one decision against the model -------------------------------------------------------------------------------------------------
SIZES = [1, 63, 65, 257, 1000]


def _scenario(name, R, n, auto):
    """Handle keywords, per-lane starting episode lengths (or None), a state override (or None) and the first decision's actions
    (or None = random) that make lanes finish at every sub-step index.  CartPole: random actions, natural termination — from lanes
    that enter the first decision 0 .. R - 1 steps into their episodes (stepped here, on the CPU, under a held push): an episode
    that starts WITH a decision falls over ~9 steps into a held push, which is sub-steps 7, 0, 1, 2 of R = 8 and never 3 .. 6.  Pendulum /
    MountainCar / Acrobot: a time limit L from {R + 1 .. 2R}, a different one per batch size, with the lanes' episode lengths staggered
    so that the first episodes end at every sub-step index ((L - 1) mod R is where all the later ones end).  MountainCarContinuous: lanes
    placed one to R steps from the goal under full throttle."""
    kw = dict(seed=SEED, auto_reset=auto, episode_stats=True, done_list=True, final_obs=auto)      # (FINAL_OBS needs AUTORESET)
    len0 = ret0 = state0 = first = None
    if name.startswith("CartPole"):
        state0, _ = model.reset_draw(name, SEED, 0, 0, n)
        len0 = (np.arange(n) % R).astype(np.int32)
        ret0 = len0.astype(F32)                                  # a reward of 1 per step taken
        for j in range(R - 1):
            stepped = model.step_once(name, state0, ((np.arange(n) // R) % 2).astype(np.int32))[0]      # a held push, either way
            state0 = np.where(len0 > j, stepped, state0).astype(state0.dtype)
    elif name in ("Pendulum", "MountainCar", "Acrobot"):
        L = R + 1 + ((SIZES.index(n) if n in SIZES else 2) * 3 + R // 2) % R
        kw["max_episode_steps"] = L
        len0 = (np.arange(n) % L).astype(np.int32)
    elif name == "MountainCarContinuous":
        k = (np.arange(n) % R) + 1                               # steps to the goal
        v = np.full(n, 0.06, F32)
        state0 = np.stack([(0.45 + 0.03 - 0.06 * k).astype(F32), v])
        first = np.ones(n, F32)
    return kw, len0, ret0, state0, first


def _check_decision(env, m, d, auto, name):
    out = env.Read()
    assert np.array_equal(env.GetState().view(np.uint8), d["state"].view(np.uint8))
    assert np.array_equal(np.ascontiguousarray(out.Observation.T).view(np.uint8), np.ascontiguousarray(d["obs"]).view(np.uint8))
    assert np.array_equal(out.Reward.view(np.uint32), d["reward"].view(np.uint32))
    assert np.array_equal(env.GetArray("done"), d["done"])
    assert np.array_equal(env.GetArray("episode_return").view(np.uint32), d["ep_ret"].view(np.uint32))
    assert np.array_equal(env.GetArray("episode_length"), d["ep_len"])
    assert np.array_equal(env.GetArray("finished_return").view(np.uint32), d["fin_ret"].view(np.uint32))
    assert np.array_equal(env.GetArray("finished_length"), d["fin_len"])
    fin = d["finished_at"] >= 0
    if d["final_obs"] is not None and auto:
        ever = d["fin_len"] > 0                                  # lanes that have finished an episode so far
        assert np.array_equal(env.GetArray("final_obs")[:, ever], d["final_obs"].astype(m.dtype)[:, ever])
    rec = env.DoneRecords()
    order = np.argsort(rec["lanes"])
    assert np.array_equal(rec["lanes"][order], np.flatnonzero(fin))                  # the done list of the DECISION: every sub-step's
    assert np.array_equal(rec["return"][order].view(np.uint32), d["fin_ret"][fin].view(np.uint32))
    assert np.array_equal(rec["length"][order], d["fin_len"][fin])
    if m.has_sbd:
        assert np.array_equal(env.GetStepsBeyondDone(), d["sbd"])
        assert env.Counters()["stepped_after_done"] == m.after_done


def _run_against_model(gpu_pkg, name, R, n, auto, decisions=40, start_tick=None, lane_offset=0, extra_kw=None, total=None):
    kw, len0, ret0, state0, first = _scenario(name, R, total or n, auto)
    if total:                                                    # a shard of a larger batch: its slice of the per-lane set-up
        sl = slice(lane_offset, lane_offset + n)
        len0, ret0, state0, first = (None if v is None else np.ascontiguousarray(v[..., sl]) for v in (len0, ret0, state0, first))
    kw.update(extra_kw or {})
    rng = np.random.default_rng(1000 * R + n + lane_offset)
    seen = np.zeros(R, np.int64)
    ever = np.zeros(n, bool)
    with _make(gpu_pkg, name, n, lane_offset=lane_offset, **kw) as env:
        env.Reset()
        if state0 is not None:
            env.SetState(state0)
        if len0 is not None:
            env.SetArray("episode_length", len0)
        if ret0 is not None:
            env.SetArray("episode_return", ret0)
        if start_tick is not None:
            env.Tick = start_tick
        m = model.RepeatModel(name, env.GetState(), SEED, lane_offset, auto, stats=True, limit=kw.get("max_episode_steps", 0), len0=len0, ret0=ret0)
        lane_steps0 = env.Counters()["lane_steps"]
        for t in range(decisions):
            a = first if (t == 0 and first is not None) else _random_actions(name, rng, n)
            tick = env.Tick
            env.StepRepeatDevice(_dev(a), R - 1)
            assert env.Tick == tick + R
            d = m.decision(a, R, tick)
            _check_decision(env, m, d, auto, name)
            f = d["finished_at"]
            seen += np.bincount(f[f >= 0], minlength=R)
            ever |= f >= 0
        assert env.Counters()["lane_steps"] == lane_steps0 + decisions * R * n     # slots: idle ones included
    return seen, ever


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("R", [2, 4, 8])
@pytest.mark.parametrize("n", SIZES)
def test_one_decision_equals_the_model(gpu_pkg, name, R, n):
    seen, ever = _run_against_model(gpu_pkg, name, R, n, auto=True)
    if n >= R:                                                   # (a lane per sub-step index: see the module docstring)
        assert (seen > 0).all(), seen                            # the freeze path ran after EVERY sub-step index
    else:
        assert seen.sum() > 0
    if name.startswith("CartPole"):
        assert ever.sum() * 4 >= n, ever.sum()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("R", [2, 4, 8])
@pytest.mark.parametrize("n", SIZES)
def test_one_decision_without_auto_reset_equals_the_model(gpu_pkg, name, R, n):
    # steps_beyond_done, the stepped-after-done counter and the reward of an already-done lane (one sub-step only) are in _check_decision
    seen, ever = _run_against_model(gpu_pkg, name, R, n, auto=False)
    if n >= R:
        assert (seen > 0).all(), seen
    else:
        assert seen.sum() > 0
    if name.startswith("CartPole"):
        assert ever.sum() * 4 >= n and seen[0] > ever.sum()      # done lanes come back and stop at sub-step 0 again


def test_double_buffer(gpu_pkg):
    seen, _ = _run_against_model(gpu_pkg, "CartPole", 4, 257, auto=True, extra_kw=dict(double_buffer=True))
    assert (seen > 0).all()
    seen, _ = _run_against_model(gpu_pkg, "Acrobot", 4, 257, auto=True, extra_kw=dict(double_buffer=True))
    assert (seen > 0).all()


@pytest.mark.parametrize("name", ["CartPole", "MountainCar"])
def test_lane_offset_two_shards_of_one_batch(gpu_pkg, name):
    # 2048 lanes = 1000 + 1048 on two handles: each shard equals its slice of the model of the whole batch (the model draws resets by
    # GLOBAL lane, so a wrong offset shows in the first reset)
    for lo, n in ((0, 1000), (1000, 1048)):
        seen, _ = _run_against_model(gpu_pkg, name, 4, n, auto=True, lane_offset=lo, total=2048, decisions=20)
        assert (seen > 0).all()


@pytest.mark.parametrize("name", ["CartPole", "CartPole64"])
def test_tick_across_2_to_the_32(gpu_pkg, name):
    seen, _ = _run_against_model(gpu_pkg, name, 4, 257, auto=True, start_tick=2 ** 32 - 3, decisions=20)
    assert (seen > 0).all()


# ---- the fused form equals single decisions ---------------------------------------------------------------------------------------
def _episode_buffers(torch, cap):
    return dict(step=torch.full((cap,), -1, dtype=torch.int32, device="cuda"), lane=torch.full((cap,), -1, dtype=torch.int32, device="cuda"),
                ret=torch.zeros(cap, dtype=torch.float32, device="cuda"), length=torch.zeros(cap, dtype=torch.int32, device="cuda"),
                capacity=cap, count=torch.zeros(2, dtype=torch.uint32, device="cuda"))


def _records(ep):
    c = ep["count"].cpu().numpy().astype(np.int64)
    k = int(c[0])
    rec = np.stack([ep["step"].cpu().numpy()[:k], ep["lane"].cpu().numpy()[:k], ep["length"].cpu().numpy()[:k]], axis=1).astype(np.int64)
    ret = ep["ret"].cpu().numpy()[:k]
    order = np.lexsort((rec[:, 1], rec[:, 0]))
    return rec[order], ret[order], c


FUSED_ROWS = [(row, row["actions"]) for row in forms.FORMS] + \
             [(row, "epsilon_greedy") for row in forms.FORMS if row["actions"] == "sample" and not model.ENVS[row["name"]][2]]


@pytest.mark.parametrize("row,actions", FUSED_ROWS, ids=[f"{r['kernel']}-{a}" for r, a in FUSED_ROWS])
def test_fused_equals_single_decisions(gpu_pkg, row, actions):
    import torch
    name, auto, shape = row["name"], row["auto_reset"], row["shape"]
    n, T, R, ring, tick0, eps, limit = 1000, 12, 3, 5, 400, 0.3, 7
    box = model.ENVS[name][2]
    adt = torch.float32 if box else torch.int32
    book = shape != "lean"
    kw = dict(seed=SEED, auto_reset=auto, lane_offset=12_345)
    if book:
        kw.update(episode_stats=True, max_episode_steps=limit, done_list=True, final_obs=auto)      # (FINAL_OBS needs AUTORESET)
    rng = np.random.default_rng(9)
    with _make(gpu_pkg, name, n, **kw) as f, _make(gpu_pkg, name, n, **kw) as e:
        policy = _dev(np.stack([_random_actions(name, rng, n) for _ in range(ring)]))
        for env in (f, e):
            env.ResetDevice()
        D = f.ObsDim
        tdt = torch.float64 if row["dtype"] == np.float64 else torch.float32
        rec_o = torch.zeros((T, D, n), dtype=tdt, device="cuda")
        rec_r = torch.zeros((T, n), dtype=torch.float32, device="cuda")
        rec_d = torch.zeros((T, n), dtype=torch.uint8, device="cuda")
        # (the actions of a plain ring rollout on a lean handle ARE the ring: d_rec_actions is refused there, as in the fused rollout)
        rec_a = torch.zeros((T, n), dtype=adt, device="cuda") if (book or actions != "ring") else None
        ep = _episode_buffers(torch, n * T) if shape == "records" else None
        torch.cuda.synchronize()
        f.RolloutFusedDevice(policy, T, n, ring, rec_obs=rec_o, rec_reward=rec_r, rec_done=rec_d, rec_actions=rec_a, actions=actions,
                             action_seed=ASEED, action_tick0=tick0, epsilon=eps, episodes=ep, repeat=R - 1)
        f.Sync()
        act = torch.empty(n, dtype=adt, device="cuda")
        want_rec, want_ret = [], []
        # the model beside the twin: the episode count the records are held to does not come from the code under test
        m = model.RepeatModel(name, e.GetState(), SEED, 12_345, auto, stats=book, limit=limit if book else 0) if ep is not None else None
        for d in range(T):
            if actions == "ring":
                act.copy_(policy[d % ring]); torch.cuda.synchronize()
            elif actions == "sample":
                e.SampleActionsDevice(act, seed=ASEED, tick=tick0 + d)
            else:
                e.ComposeActionsDevice(policy[d % ring], eps, act, seed=ASEED, tick=tick0 + d)
            tick = e.Tick
            e.StepRepeatDevice(act, R - 1)
            e.Sync()
            o = e.Read()
            if m is not None:
                md = m.decision(act.cpu().numpy(), R, tick)
                assert np.array_equal(e.GetArray("done"), md["done"]), d
            if rec_a is not None:
                assert np.array_equal(rec_a[d].cpu().numpy().view(np.uint32), act.cpu().numpy().view(np.uint32)), d
            assert np.array_equal(rec_o[d].cpu().numpy(), o.Observation.T), d
            assert np.array_equal(rec_r[d].cpu().numpy().view(np.uint32), o.Reward.view(np.uint32)), d
            assert np.array_equal(rec_d[d].cpu().numpy(), e.GetArray("done")), d
            if book:
                r = e.DoneRecords()
                for lane, ret, ln in zip(r["lanes"], r["return"], r["length"]):
                    want_rec.append((d, int(lane), int(ln))); want_ret.append(float(ret))
        assert np.array_equal(f.GetState(), e.GetState()) and f.Tick == e.Tick
        assert f.Counters()["lane_steps"] == e.Counters()["lane_steps"]
        for arr in ("reward", "done") + (("episode_return", "episode_length", "finished_return", "finished_length") if book else ()) + (("final_obs",) if book and auto else ()):
            assert np.array_equal(f.GetArray(arr), e.GetArray(arr)), arr
        if name.startswith("CartPole") and not auto:
            assert np.array_equal(f.GetStepsBeyondDone(), e.GetStepsBeyondDone())
            assert f.Counters()["stepped_after_done"] == e.Counters()["stepped_after_done"]
        if book:
            a, b = f.DoneRecords(), e.DoneRecords()                                 # "the most recent step" = the rollout's last DECISION
            oa, ob = np.argsort(a["lanes"]), np.argsort(b["lanes"])
            for k in ("lanes", "return", "length") + (("final_obs",) if auto else ()):
                assert np.array_equal(a[k][oa], b[k][ob]), k
            assert len(want_rec) > 0
        if ep is not None:
            got_rec, got_ret, counts = _records(ep)
            want = np.array(want_rec, dtype=np.int64).reshape(-1, 3)
            order = np.lexsort((want[:, 1], want[:, 0]))
            assert counts[0] == counts[1] == m.episodes == len(want)
            assert np.array_equal(got_rec, want[order])                              # the DECISION index is the record's step index
            assert np.array_equal(got_ret.view(np.uint32), np.array(want_ret, F32)[order].view(np.uint32))


def test_fused_records_with_a_capacity_one_below_the_count(gpu_pkg):
    import torch
    n, T, R = 1000, 12, 3
    kw = dict(seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=7)
    with _make(gpu_pkg, "CartPole", n, **kw) as f, _make(gpu_pkg, "CartPole", n, **kw) as g:
        f.ResetDevice(); g.ResetDevice()
        full = _episode_buffers(torch, n * T)
        torch.cuda.synchronize()
        f.RolloutFusedDevice(None, T, actions="sample", action_seed=ASEED, episodes=full, repeat=R - 1)
        f.Sync()
        rec, ret, counts = _records(full)
        total = int(counts[1])
        assert counts[0] == total > n                           # every lane truncates at env step 7 at the latest: 36 steps, > 1 episode each
        short = _episode_buffers(torch, total - 1)
        torch.cuda.synchronize()
        g.RolloutFusedDevice(None, T, actions="sample", action_seed=ASEED, episodes=short, repeat=R - 1)
        g.Sync()
        rec2, ret2, counts2 = _records(short)
        assert counts2.tolist() == [total - 1, total]
        have = {tuple(r) for r in rec.tolist()}
        assert len({tuple(r) for r in rec2.tolist()}) == total - 1 and {tuple(r) for r in rec2.tolist()} <= have
        assert np.array_equal(f.GetState(), g.GetState())


# ---- attachments at the Images runner's SkippedFrames = 1 ------------------------------------------------------------------------
RUNNER = ((200, 150, 200, 150), (40, 20))
ATT = dict(seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=9)


def _gray(env, crop, size):
    import torch
    out = torch.empty((env.NumberOfEnvironments, size[1], size[0]), dtype=torch.uint8, device="cuda")
    env.RenderDevice(out, "gray", crop=crop, size=size)
    env.Sync()
    return out.cpu().numpy()


def test_pixel_stack_restarts_a_lane_that_finished_mid_decision(gpu_pkg):
    n = 257
    crop, size = RUNNER
    rng = np.random.default_rng(2)
    with gpu_pkg.VectorEnv("CartPole-v1", n, **ATT) as env:
        env.Reset()
        st = env.PixelStack(depth=2, size=size, crop=crop, format="gray8")
        m = stack_model.PixelStackModel(_gray(env, crop, size), 2)
        cp = model.RepeatModel("CartPole", env.GetState(), SEED, 0, True, stats=True, limit=9)
        mid = 0
        for t in range(30):
            a = rng.integers(0, 2, n).astype(np.int32)
            tick = env.Tick
            st.Step(_dev(a), repeat=1)
            d = cp.decision(a, 2, tick)
            done = env.GetArray("done")
            assert np.array_equal(done, d["done"]) and np.array_equal(env.GetState(), d["state"])
            m.push(_gray(env, crop, size), done)                 # the per-decision observation (rendered) and done byte
            assert np.array_equal(st.Tensor.cpu().numpy(), m.stack), t
            first = d["finished_at"] == 0                        # finished at sub-step 0, idle at sub-step 1
            mid += int(first.sum())
            assert (done[first] != 0).all()
        assert mid > 0


def test_episode_memory_rows_are_decisions(gpu_pkg):
    n = 257
    rng = np.random.default_rng(3)
    with gpu_pkg.VectorEnv("CartPole-v1", n, **ATT) as env:
        obs = env.Reset()
        mem = env.EpisodeMemory(capacity=40, max_length=0, history=4)
        m = memory_model.EpisodeMemoryModel(obs, 40, 9, 4)
        cp = model.RepeatModel("CartPole", env.GetState(), SEED, 0, True, stats=True, limit=9)
        for t in range(30):
            a = memory_model.mixed_policy(n, rng, t, 2)
            tick = env.Tick
            mem.Step(_dev(a), repeat=1)
            d = cp.decision(a, 2, tick)
            out = env.Read()
            assert np.array_equal(out.Reward.view(np.uint32), d["reward"].view(np.uint32))      # the SUMMED reward
            m.push(a, d["reward"], d["done"], out.Observation, env.Tick)
            got, want = mem.Episodes(), m.kept()
            for g, w, what in zip(got, want, ("return", "length", "end_tick", "lane")):
                assert np.array_equal(g, w), (what, t)
        assert m.ended > n
        x, a_, oh, r = m.dataset_params(2)
        gx, ga, goh, gr = (v.cpu().numpy() for v in mem.BuildDataset("params", min_episodes=0, reward=True))
        assert len(x) > 0 and np.array_equal(gx, x) and np.array_equal(gr.view(np.uint32), r.view(np.uint32))
        assert np.array_equal(ga, a_.astype(ga.dtype)) and np.array_equal(goh, oh)


def test_actor_step_with_repeat_equals_the_unfused_loop(gpu_pkg):
    n = 257
    rng = np.random.default_rng(4)
    widths, flat, net = actor_twin.net(rng, [2 * 4, 16, 2])
    with gpu_pkg.VectorEnv("CartPole-v1", n, **ATT) as f, gpu_pkg.VectorEnv("CartPole-v1", n, **ATT) as e:
        f.Reset(); e.Reset()
        fa, ea = f.Actor(net, history=2), e.Actor(net, history=2)
        for d in range(30):
            got = fa.Step(0.2, ASEED, d, repeat=1)
            want = ea.Act(0.2, ASEED, d)
            e.StepRepeatDevice(want, 1)
            ea.Push()
            f.Sync(); e.Sync()
            assert np.array_equal(got.cpu().numpy(), want.cpu().numpy()), d
            assert np.array_equal(f.GetState(), e.GetState()) and f.Tick == e.Tick == 1 + 2 * (d + 1)
            assert np.array_equal(fa.History(), ea.History()), d
        assert (f.GetArray("finished_length") > 0).any()


def test_pushes_after_more_than_one_decision_stay_refused(gpu_pkg):
    import torch
    n = 257
    rng = np.random.default_rng(6)
    widths, flat, net = actor_twin.net(rng, [2 * 4, 8, 2])
    inv = gpu_pkg._capi.ERR_INVALID_ARG
    with gpu_pkg.VectorEnv("CartPole-v1", n, **ATT) as env:
        env.Reset()
        mem = env.EpisodeMemory(capacity=8, history=2)
        ac = env.Actor(net, history=2)
        lib, h = env._lib, env._h
        ring = _dev(rng.integers(0, 2, (2, n)).astype(np.int32))
        mem.Step(ring[0], repeat=1); ac.Push()                   # one decision: both accepted
        before, stats = mem.Episodes(), mem.Stats()
        hist = ac.History()
        for launch in (lambda: env.RolloutFusedDevice(ring, 2, n, 2), lambda: env.RolloutFusedDevice(ring, 2, n, 2, repeat=1)):
            launch()
            assert lib.gymnet_vecenv_memory_push_device(h, C.c_void_p(ring.data_ptr()), None) == inv
            assert b"exactly one" in lib.gymnet_last_error() or b"single" in lib.gymnet_last_error()
            assert lib.gymnet_vecenv_actor_push_device(h, None) == inv
            assert b"exactly one" in lib.gymnet_last_error() or b"single" in lib.gymnet_last_error()
            poisoned = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            assert lib.gymnet_vecenv_actor_act_device(h, C.c_void_p(poisoned.data_ptr()), None, C.c_float(0.0), 0, 0) == inv   # stale history
            env.Sync()
            assert (poisoned.cpu().numpy() == 0x5A5A5A5A).all()
            assert all(np.array_equal(x, y) for x, y in zip(before, mem.Episodes())) and mem.Stats() == stats
            assert np.array_equal(ac.History(), hist)
            mem.Reset(); ac.Reset()
            before, stats, hist = mem.Episodes(), mem.Stats(), ac.History()
        env.RolloutFusedDevice(ring, 1, n, 2, repeat=1)          # ONE decision through the fused call: accepted
        mem.Push(ring[0]); ac.Push()


# ---- refusals and the host boundary ----------------------------------------------------------------------------------------------
def test_refusals(gpu_pkg):
    capi = gpu_pkg._capi
    n = 64
    rng = np.random.default_rng(8)
    widths, flat, net = actor_twin.net(rng, [4, 8, 2])
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True) as env:
        env.Reset()
        lib, h = env._lib, env._h
        a = _dev(np.zeros(n, np.int32))
        host = np.zeros(n, np.int32)
        obs, rew, done = np.full((n, 4), 7, F32), np.full(n, 7, F32), np.full(n, 7, np.uint8)
        state, tick = env.GetState(), env.Tick
        spec = capi.RolloutSpec(struct_size=C.sizeof(capi.RolloutSpec), action_source=capi.ACTIONS_RING, d_actions=a.data_ptr(), steps=2,
                                action_stride=0, ring=1)
        for bad in (256, -1):
            assert lib.gymnet_vecenv_step_repeat_device(h, C.c_void_p(a.data_ptr()), bad) == capi.ERR_INVALID_ARG
            assert b"[0, 255]" in lib.gymnet_last_error()
            assert lib.gymnet_vecenv_step_repeat(h, host.ctypes.data_as(C.c_void_p), bad, obs.ctypes.data_as(C.c_void_p),
                                                 rew.ctypes.data_as(C.c_void_p), done.ctypes.data_as(C.c_void_p)) == capi.ERR_INVALID_ARG
            assert lib.gymnet_vecenv_rollout_repeat_device(h, C.byref(spec), bad) == capi.ERR_INVALID_ARG
        assert (obs == 7).all() and (rew == 7).all() and (done == 7).all()
        spec.steps = 2 ** 30                                     # T * R = 2^31 does not fit an int32
        assert lib.gymnet_vecenv_rollout_repeat_device(h, C.byref(spec), 1) == capi.ERR_INVALID_ARG
        assert b"int32" in lib.gymnet_last_error()
        env.Actor(net, history=1)
        spec.steps, spec.action_source = 2, capi.ACTIONS_ACTOR
        assert lib.gymnet_vecenv_rollout_repeat_device(h, C.byref(spec), 1) == capi.ERR_UNSUPPORTED
        assert b"unfused loop" in lib.gymnet_last_error()
        assert np.array_equal(env.GetState(), state) and env.Tick == tick
        assert lib.gymnet_vecenv_rollout_repeat_device(h, C.byref(spec), 0) == 0          # repeat = 0 forwards to the actor rollout
        assert env.Tick == tick + 2
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True, validate_actions=True) as env:
        env.Reset()
        state = env.GetState()
        with pytest.raises(gpu_pkg.InvalidActionError):
            env.StepRepeatDevice(_dev(np.full(n, 2, np.int32)), 3)                      # validates as StepDevice does
        assert np.array_equal(env.GetState(), state)
        env.StepRepeatDevice(_dev(np.ones(n, np.int32)), 3)
        assert env.Tick == 5


@pytest.mark.parametrize("name", ["CartPole", "CartPole64", "Pendulum"])
@pytest.mark.parametrize("n", [33, 5000])
def test_host_boundary_returns_what_the_device_call_leaves(gpu_pkg, name, n):
    rng = np.random.default_rng(n)
    kw = dict(seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=5)
    with _make(gpu_pkg, name, n, **kw) as f, _make(gpu_pkg, name, n, **kw) as e:
        f.Reset(); e.Reset()
        for t in range(6):
            a = _random_actions(name, rng, n)
            x = f.StepRepeat(a, 2)
            e.StepRepeatDevice(_dev(a), 2)
            y = e.Read()
            assert np.array_equal(x.Observation, y.Observation) and np.array_equal(x.Reward.view(np.uint32), y.Reward.view(np.uint32))
            assert np.array_equal(x.Done, y.Done) and np.array_equal(x.Truncated, y.Truncated) and f.Tick == e.Tick


def test_resident_handle_leaves_residency_for_a_held_step(gpu_pkg):
    n = 8
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True, resident=True) as f, \
            gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True) as e:
        f.Reset(); e.Reset()
        a = np.arange(n, dtype=np.int32) % 2
        for t in range(3):
            x, y = f.Step(a), e.Step(a)
            assert np.array_equal(x.Observation, y.Observation)
            x, y = f.StepRepeat(a, 3), e.StepRepeat(a, 3)
            assert np.array_equal(x.Observation, y.Observation) and np.array_equal(x.Reward, y.Reward) and f.Tick == e.Tick
