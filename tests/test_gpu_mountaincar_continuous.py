"""MountainCarContinuous-v0 on the GPU (upstream gym continuous_mountain_car.py; absent from the reference).

1. Teacher-forced steps from the golden states (tests/golden/mountaincar_continuous.npz, the float64 restatement): state <= 1e-6,
   reward <= 1e-5, done exact except positions within 1e-6 of the goal.
2. The goal threshold: start states whose next position is exactly 0x3EE66666 (below 0.45: not done) or 0x3EE66667 (done).
3. Every recipe of tests/_mountaincar_continuous_matrix.py replayed against the float32 twin BIT FOR BIT: state, observation, reward,
   done byte (bit 1 = the time limit), done list, dense episode views, terminal observations, sorted rollout episode records.
4. Out-of-range and special actions: the clamp feeds the force, the raw action the reward.
5. Closed loop: an energy-pumping policy reaches the goal on every lane, in the twin's number of steps.
6. The façade, the resident path and the generic C-ABI behaviour (render / float64 / epsilon-greedy refused, VALIDATE_ACTIONS a no-op,
   checkpoint and state round trips).
7. A group of two members on one device equals one handle over the same global lanes."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mountaincar_continuous_matrix as MC  # noqa: E402
import _mountaincar_continuous_twin as tw  # noqa: E402

pytestmark = pytest.mark.gpu
GYM = tw.GYM
SEED, ASEED = 0x5EED, 0xAC710
STEPS, T_ROLLOUT, RING = 18, 16, 5
KEYS = np.array([0x1234567, 0x9ABCDEF0123, 77], dtype=np.uint64)     # per-lane Philox keys: lane i gets KEYS[i % 3]
F32 = np.float32

RECIPES = MC.recipes()


@pytest.fixture(autouse=True)
def _oracle_built(oracle):
    """The twin's cos and reset draws come from the oracle's C restatement: build it once."""
    return oracle


def _eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _first_diff(a, b):
    d = np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))
    return None if len(d) == 0 else (tuple(int(x) for x in d[0]), a[tuple(d[0])], b[tuple(d[0])])


def _by(fam):
    return [pytest.param(r, id=r["name"]) for r in RECIPES if r["family"] == fam]


def _lane_seeds(n):
    return KEYS[np.arange(n) % 3]


# ---- 1. teacher-forced against the golden file ---------------------------------------------------------------------------------
def test_teacher_forced_steps_match_the_float64_restatement(gpu_pkg, golden):
    g = golden("mountaincar_continuous")
    n = g["state"].shape[1]
    with gpu_pkg.VectorEnv(GYM, n, seed=SEED) as env:
        env.Reset()
        env.SetState(g["state"])
        out = env.Step(g["action"])
        got = env.GetState()
    assert np.abs(got.astype(np.float64) - g["next_state"]).max() <= 1e-6
    assert np.abs(out.Reward.astype(np.float64) - g["reward"]).max() <= 1e-5
    near = np.abs(g["next_state"][0] - 0.45) < 1e-6
    assert np.array_equal(out.Done[~near], g["done"].astype(bool)[~near])
    assert _eq(out.Observation, got.T)
    s, rw, d = tw.step_f32(g["state"], g["action"])                   # and the kernel is its float32 twin, bit for bit
    assert _eq(got, s) and _eq(out.Reward, rw) and _eq(out.Done, d)


# ---- 2. the goal threshold -----------------------------------------------------------------------------------------------------
def _threshold_starts(rng, target_bits, count):
    """Float32 (state, action) pairs whose next position is EXACTLY the float32 with bits target_bits, with v >= 0 (found with the twin)."""
    target = np.array([target_bits], np.uint32).view(F32)[0]
    states, acts = [], []
    for _ in range(100000):
        if len(states) == count:
            break
        p0 = F32(rng.uniform(0.39, 0.449))
        a = F32(rng.choice([0.0, 1.0, -1.0, 3.0, rng.uniform(-1, 1)]))
        v1 = F32(target - p0)                                         # exact (Sterbenz): p0 + v1 == target exactly
        if not (F32(0) <= v1 <= F32(0.07)):
            continue
        force = F32(min(max(a, F32(-1)), F32(1)))
        delta = F32(force * F32(0.0015)) - F32(F32(0.0025) * tw.kcos(np.array([F32(3) * p0]))[0])
        v0 = F32(v1 - delta)
        for cand in (v0, np.nextafter(v0, F32(1)), np.nextafter(v0, F32(-1))):
            s, _, _ = tw.step_f32(np.array([[p0], [cand]], F32), np.array([a], F32))
            if s[0].view(np.uint32)[0] == target_bits and s[1, 0] >= 0:
                states.append((p0, cand)); acts.append(a)
                break
    assert len(states) == count
    return np.array(states, F32).T, np.array(acts, F32)


def test_goal_threshold_edge_vectors(gpu_pkg):
    rng = np.random.default_rng(45)
    below, a_below = _threshold_starts(rng, 0x3EE66666, 48)
    at, a_at = _threshold_starts(rng, 0x3EE66667, 48)
    s0, a = np.concatenate([below, at], axis=1), np.concatenate([a_below, a_at])
    with gpu_pkg.VectorEnv(GYM, s0.shape[1], seed=SEED) as env:
        env.Reset()
        env.SetState(s0)
        out = env.Step(a)
        got = env.GetState()
    bits = got[0].view(np.uint32)
    assert (bits[:48] == 0x3EE66666).all() and (bits[48:] == 0x3EE66667).all() and (got[1] >= 0).all()
    assert not out.Done[:48].any() and out.Done[48:].all()           # (double)p >= 0.45 exactly
    assert (got[0, :48].astype(np.float64) < 0.45).all() and (got[0, 48:].astype(np.float64) >= 0.45).all()
    s, rw, _ = tw.step_f32(s0, a)
    assert _eq(got, s) and _eq(out.Reward, rw)


# ---- 3. the recipe table -------------------------------------------------------------------------------------------------------
def _start(r, rng):
    """Float32 start state [2, n] and the lanes that must finish at step 0 / must not (the last wave all, the second wave none)."""
    n, lanes = r["n"], 64 * r["vec"]
    fin = np.arange((n - 1) // lanes * lanes, n)
    if len(fin) < lanes // 2 and n > 3 * lanes:
        fin = np.arange(max(0, fin[0] - lanes), n)
    keep = np.arange(lanes, min(2 * lanes, fin[0]))
    s = np.stack([rng.uniform(-0.6, -0.4, n), rng.uniform(-0.01, 0.01, n)])
    edge = rng.random(n) < 0.25                                        # near the goal: some finish during the replay
    wall = (rng.random(n) < 0.05) & ~edge                             # against the left wall
    edge[keep] = wall[keep] = False
    s[:, edge] = np.stack([rng.uniform(0.43, 0.5, edge.sum()), rng.uniform(0.0, 0.07, edge.sum())])
    s[:, wall] = np.stack([rng.uniform(-1.2, -1.15, wall.sum()), rng.uniform(-0.07, -0.03, wall.sum())])
    s[:, fin] = np.stack([rng.uniform(0.47, 0.5, len(fin)), rng.uniform(0.04, 0.07, len(fin))])      # past the goal whatever the push
    return s.astype(F32), fin, keep


def _actions(rng, n):
    a = rng.uniform(-1.5, 1.5, n).astype(F32)
    a[rng.random(n) < 0.05] = -0.0
    far = rng.random(n) < 0.05                                         # beyond the bounds: clamped for the force, raw in the reward
    a[far] = rng.choice(F32([-50.0, 3.0, -1.0000001, 1.0000001]), far.sum())
    return a


def _open(gpu_pkg, r, **more):
    kw = dict(seed=SEED, auto_reset=r["auto_reset"], lane_offset=r["lane_offset"], done_list=r["done_list"], episode_stats=r["episode_stats"],
              final_obs=r["final_obs"], max_episode_steps=r["max_episode_steps"], double_buffer=r["double_buffer"], resident=r["resident"])
    kw.update(more)
    return gpu_pkg.VectorEnv(GYM, r["n"], **kw)


def _prepare(env, r, rng):
    """Seeds, the reset (checked against the reset twin), the forced start state and running statistics; returns the Replay."""
    seeds = _lane_seeds(r["n"]) if r["lane_seeds"] else None
    if seeds is not None:
        env.Seed(seeds.astype(np.int64))
    tick = env.Tick
    if r["resident"]:
        env.Reset()
    else:
        env.ResetDevice()
    assert _eq(env.GetState(), tw.reset(SEED, r["lane_offset"], tick, r["n"], seeds))
    s0, must, keep = _start(r, rng)
    env.SetState(s0)
    ln0 = ret0 = None
    if r["episode_stats"]:
        ln0 = rng.integers(0, max(r["max_episode_steps"], 6), r["n"]).astype(np.int32)
        if r["max_episode_steps"]:
            ln0[keep] = 0
        ret0 = rng.uniform(-3, 3, r["n"]).astype(F32)
        env.SetArray("episode_length", ln0)
        env.SetArray("episode_return", ret0)
    rp = tw.Replay(env.GetState(), SEED, r["lane_offset"], r["auto_reset"], r["episode_stats"], r["max_episode_steps"], r["final_obs"],
                   seeds, ln0, ret0)
    assert _eq(rp.s, s0)
    return rp, must, keep


def _check_dense(env, r, rp):
    if r["episode_stats"]:
        assert _eq(env.GetArray("episode_length"), rp.ln) and _eq(env.GetArray("episode_return"), rp.ret)
        if not r["resident"]:
            assert _eq(env.GetArray("finished_length"), rp.fin_len) and _eq(env.GetArray("finished_return"), rp.fin_ret)
    if r["final_obs"]:
        assert _eq(env.GetArray("final_obs"), rp.final)


@pytest.mark.parametrize("r", _by("step_kernel"))
def test_step_instantiation_equals_the_twin(gpu_pkg, r):
    rng = np.random.default_rng(zlib.crc32(r["name"].encode()))
    with _open(gpu_pkg, r, launch_policy=r["launch"]) as env:
        rp, must, keep = _prepare(env, r, rng)
        assert env.KernelName() == r["name"]
        pol = env.GetLaunchPolicy()
        assert all(pol[k] == v for k, v in r["launch"].items()), (pol, r["launch"])
        for t in range(STEPS):
            a = _actions(rng, r["n"])
            tick = env.Tick
            out = env.Step(a)
            obs, rw, db, fin = rp.step(a, tick)
            if t == 0:
                assert fin[must].all() and not fin[keep].any()
            assert _eq(env.GetState(), rp.s), (t, _first_diff(env.GetState(), rp.s))
            assert _eq(out.Observation, obs.T) and _eq(out.Reward, rw) and _eq(env.GetArray("done"), db), t
            if r["done_list"]:
                assert _eq(np.sort(env.DoneLanes()), np.nonzero(fin)[0]), t
                rec = env.DoneRecords()
                order = np.argsort(rec["lanes"])
                if r["episode_stats"]:
                    assert _eq(rec["return"][order], rp.fin_ret[fin]) and _eq(rec["length"][order], rp.fin_len[fin]), t
                if r["final_obs"]:
                    assert _eq(rec["final_obs"][order], rp.final[:, fin].T), t
        assert env.KernelName() == r["name"]
        _check_dense(env, r, rp)


def _episode_buffers(torch, cap, no_overflow):
    ep = dict(step=torch.full((cap,), -1, dtype=torch.int32, device="cuda"), lane=torch.full((cap,), -1, dtype=torch.int32, device="cuda"),
              ret=torch.zeros(cap, dtype=torch.float32, device="cuda"), length=torch.zeros(cap, dtype=torch.int32, device="cuda"),
              capacity=cap, count=torch.zeros(2, dtype=torch.uint32, device="cuda"))
    if no_overflow:
        ep["no_overflow"] = True
    return ep


@pytest.mark.parametrize("r", _by("rollout_kernel"))
def test_rollout_instantiation_equals_the_twin(gpu_pkg, r):
    import torch
    rng = np.random.default_rng(zlib.crc32(r["name"].encode()))
    n, T, v, src = r["n"], T_ROLLOUT, r["vec"], r["actions"]
    with _open(gpu_pkg, r, launch_policy=r["launch"]) as env:
        rp, must, keep = _prepare(env, r, rng)
        ring = torch.from_numpy(np.stack([_actions(rng, n) for _ in range(RING)])).cuda() if src == "ring" else None
        rec_o = torch.zeros((T, 2, n), dtype=torch.float32, device="cuda")
        rec_r = torch.zeros((T, n), dtype=torch.float32, device="cuda")
        rec_d = torch.zeros((T, n), dtype=torch.uint8, device="cuda")
        rec_a = torch.zeros((T, n), dtype=torch.float32, device="cuda") if r["rec_actions"] else None
        cap = max(n * T, 128 * 64 * v * T) if r["records"] == "no_overflow" else n * T
        ep = _episode_buffers(torch, cap, r["records"] == "no_overflow") if r["records"] != "none" else None
        bufs = [x for x in (ring, rec_o, rec_r, rec_d, rec_a) if x is not None]
        assert all(b.data_ptr() % 16 == 0 for b in bufs)                # the preconditions of the intended width
        assert v == 1 or (n % v == 0 and (ring is None or ring.stride(0) % v == 0))
        pol = env.GetLaunchPolicy()
        name, got_v = MC.rollout_instantiation(pol["vec"], n, r["auto_reset"], r["name"].split(",")[3] == "true", src, ep is not None,
                                               r["records"] == "no_overflow", pol["reset_form"], action_stride=r["action_stride"])
        assert name == r["name"] and got_v == v
        tick0, atick0 = env.Tick, 1000 + r["lane_offset"] % 7
        torch.cuda.synchronize()
        env.RolloutFusedDevice(ring, T, n if ring is not None else 0, RING, rec_obs=rec_o, rec_reward=rec_r, rec_done=rec_d, rec_actions=rec_a,
                               actions=src, action_seed=ASEED, action_tick0=atick0, episodes=ep)
        env.Sync()
        assert env.Tick == tick0 + T
        got_o, got_r, got_d = rec_o.cpu().numpy(), rec_r.cpu().numpy(), rec_d.cpu().numpy()
        got_a = rec_a.cpu().numpy() if rec_a is not None else None
        acts = ring.cpu().numpy() if ring is not None else None
        want, want_ret = [], []
        for t in range(T):
            a = acts[t % RING] if src == "ring" else tw.box_sample(ASEED, r["lane_offset"], atick0 + t, n)
            if got_a is not None:
                assert _eq(got_a[t], a), t
            obs, rw, db, fin = rp.step(a, tick0 + t)
            assert _eq(got_o[t], obs), (t, _first_diff(got_o[t], obs))
            assert _eq(got_r[t], rw) and _eq(got_d[t], db), t
            lanes = np.nonzero(fin)[0]
            want.append(np.stack([np.full(len(lanes), t), lanes, rp.fin_len[fin] if rp.stats else np.zeros(len(lanes), np.int32)], axis=1))
            want_ret.append(rp.fin_ret[fin].copy())
        assert _eq(env.GetState(), rp.s), _first_diff(env.GetState(), rp.s)
        _check_dense(env, r, rp)
        if r["done_list"]:
            assert _eq(np.sort(env.DoneLanes()), lanes)                  # the done list describes the rollout's last step
        if ep is not None:
            c = ep["count"].cpu().numpy().astype(np.int64)
            k = int(c[0])
            rec = np.stack([ep["step"].cpu().numpy()[:k], ep["lane"].cpu().numpy()[:k], ep["length"].cpu().numpy()[:k]], axis=1)
            got_ret = ep["ret"].cpu().numpy()[:k]
            order = np.lexsort((rec[:, 1], rec[:, 0]))
            want = np.concatenate(want)
            assert c[0] == c[1] == len(want) > 0
            assert _eq(rec[order], want) and _eq(got_ret[order], np.concatenate(want_ret))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("r", _by("resident_kernel"))
def test_resident_instantiation_equals_the_twin(gpu_pkg, r):
    rng = np.random.default_rng(zlib.crc32(r["name"].encode()))
    with _open(gpu_pkg, r) as env:
        rp, must, keep = _prepare(env, r, rng)
        for t in range(STEPS):
            a = _actions(rng, r["n"])
            tick = env.Tick
            out = env.Step(a)
            obs, rw, db, fin = rp.step(a, tick)
            if t == 0:
                assert fin[must].all()
            assert _eq(out.Observation, obs.T) and _eq(out.Reward, rw) and _eq(out.Done, fin) and _eq(out.Truncated, (db & 2) != 0), t
        assert env.Tick == tick + 1
        assert _eq(env.GetState(), rp.s)
        _check_dense(env, r, rp)


# ---- 4. special actions --------------------------------------------------------------------------------------------------------
def test_out_of_range_and_special_actions(gpu_pkg):
    specials = F32([-0.0, 3.0, -3.0, np.inf, -np.inf, np.nan, 1.0, -1.0])
    k = len(specials)
    s0 = np.stack([np.concatenate([np.full(k, -0.5), np.full(k, 0.48)]), np.concatenate([np.zeros(k), np.full(k, 0.05)])]).astype(F32)
    a = np.concatenate([specials, specials])                          # the first k lanes mid-valley, the last k past the goal
    with gpu_pkg.VectorEnv(GYM, 2 * k, seed=SEED) as env:
        env.Reset()
        env.SetState(s0)
        out = env.Step(a)
        got = env.GetState()
    s, rw, d = tw.step_f32(s0, a)
    assert _eq(got, s) and _eq(out.Reward, rw) and _eq(out.Done, d)
    r, fin = out.Reward, out.Done
    assert not fin[:k].any() and fin[k:k + 5].all() and not fin[k + 5]            # NaN force: NaN state, never done
    assert r[0] == 0.0 and not np.signbit(r[0]) and r[k] == 100.0                 # a = -0.0: no action cost
    assert abs(r[1] + 0.9) < 1e-6 and abs(r[2] + 0.9) < 1e-6                      # a = +-3: the RAW action in the reward
    assert abs(r[k + 1] - 99.1) < 1e-5 and abs(r[k + 2] - 99.1) < 1e-5
    assert np.isneginf(r[[3, 4, k + 3, k + 4]]).all()                             # +-inf: clamped force, -inf reward
    assert np.isfinite(got[:, [3, 4, k + 3, k + 4]]).all()
    assert np.isnan(r[[5, k + 5]]).all() and np.isnan(got[:, [5, k + 5]]).all()   # NaN passes through the clamp
    # the clamp: +-3 and +-inf push exactly like +-1
    assert _eq(got[:, [1, 3]], got[:, [6, 6]]) and _eq(got[:, [2, 4]], got[:, [7, 7]])


# ---- 5. closed loop ------------------------------------------------------------------------------------------------------------
def test_energy_pumping_policy_reaches_the_goal_in_the_twins_steps(gpu_pkg):
    n, limit = 256, 999
    with gpu_pkg.VectorEnv(GYM, n, seed=SEED) as env:
        tick = env.Tick
        obs = env.Reset()
        s = tw.reset(SEED, 0, tick, n)
        assert _eq(obs, s.T)
        first = np.full(n, -1)
        twin_first = np.full(n, -1)
        for t in range(limit):
            a = np.where(obs[:, 1] >= 0, F32(1), F32(-1)).astype(F32)    # a = sign(v), a = 1 at v = 0
            out = env.Step(a)
            s, _, d = tw.step_f32(s, a)
            obs = out.Observation
            assert _eq(obs, s.T), t
            first[(first < 0) & out.Done] = t + 1
            twin_first[(twin_first < 0) & d] = t + 1
            if (first > 0).all():
                break
    assert (first > 0).all() and first.max() < limit
    assert np.array_equal(first, twin_first)


# ---- 6. façade, resident path, generic behaviour -------------------------------------------------------------------------------
def test_facade_reset_step_and_time_limit(gpu_pkg):
    with gpu_pkg.MountainCarContinuousEnv(seed=SEED, max_episode_steps=3) as env:
        assert isinstance(env.ActionSpace, gpu_pkg.Box) and env.RewardRange == (-np.inf, 100.0)
        tick = env._v.Tick
        o = env.Reset()
        s = tw.reset(SEED, 0, tick, 1)
        assert o.dtype == np.float32 and o.shape == (2,) and _eq(o, s[:, 0])
        for t, a in enumerate((0.25, 3.0, -0.5)):
            st = env.Step(a)
            s, rw, _ = tw.step_f32(s, np.array([a], F32))
            assert _eq(st.Observation, s[:, 0]) and st.Reward == rw[0]
            assert st.Done == (t == 2)
            assert st.Information == ({"TimeLimit.truncated": True} if t == 2 else None)
        assert env.Render() is None
        with pytest.raises(NotImplementedError):                      # GYMNET_ERR_UNSUPPORTED: frames exist for CartPole only
            env.Render("rgb_array")


def test_resident_facade_is_bit_identical_to_the_launch_path(gpu_pkg):
    rng = np.random.default_rng(8)
    acts = rng.uniform(-1.2, 1.2, 300).astype(F32)
    runs = []
    for resident in (False, True):
        got = []
        with gpu_pkg.MountainCarContinuousEnv(seed=SEED, resident=resident) as env:
            got.append(env.Reset())
            for a in acts:
                st = env.Step(float(a))
                got.append((st.Observation, st.Reward, st.Done))
                if st.Done:
                    got.append(env.Reset())
        runs.append(got)
    assert len(runs[0]) == len(runs[1])
    for x, y in zip(*runs):
        if isinstance(x, tuple):
            assert _eq(x[0], y[0]) and x[1] == y[1] and x[2] == y[2]
        else:
            assert _eq(x, y)


def test_float64_render_and_epsilon_greedy_are_unsupported(gpu_pkg):
    capi = gpu_pkg._capi
    lib = capi.load_library()
    cfg = capi.Config(struct_size=C.sizeof(capi.Config), env_id=capi.ENV_IDS[GYM], num_envs=8, device=0, flags=capi.FLAG_F64, seed=1)
    h = C.c_void_p()
    assert lib.gymnet_vecenv_create(C.byref(cfg), C.byref(h)) == capi.ERR_UNSUPPORTED and not h.value
    with pytest.raises(NotImplementedError):
        gpu_pkg.VectorEnv(GYM, 8, dtype=np.float64)
    import torch
    with gpu_pkg.VectorEnv(GYM, 256, seed=SEED, auto_reset=True) as env:
        env.ResetDevice()
        with pytest.raises(NotImplementedError):
            env.Render("rgb_array")
        pol = torch.zeros(256, dtype=torch.float32, device="cuda")
        out = torch.zeros(256, dtype=torch.float32, device="cuda")
        with pytest.raises(NotImplementedError):
            env.ComposeActionsDevice(pol, 0.5, out)
        with pytest.raises(NotImplementedError):
            env.RolloutFusedDevice(pol, 4, 256, 1, actions="epsilon_greedy", epsilon=0.5)
        # ActionSpace.Sample() on the device is Box(-1, 1)'s uniform draw
        assert _eq(env.SampleActions(seed=ASEED, tick=3), tw.box_sample(ASEED, 0, 3, 256))


def test_validate_actions_is_a_no_op(gpu_pkg):
    n = 64
    rng = np.random.default_rng(2)
    a = rng.uniform(-1, 1, n).astype(F32)
    a[::5] = 7.0
    a[1::5] = -40.0
    outs = []
    for validate in (False, True):
        with gpu_pkg.VectorEnv(GYM, n, seed=SEED, validate_actions=validate) as env:
            env.Reset()
            out = env.Step(a)
            outs.append((env.GetState(), out.Reward, out.Done))
    assert all(_eq(x, y) for x, y in zip(*outs))


def test_checkpoint_restore_and_state_round_trips(gpu_pkg):
    n = 3000
    rng = np.random.default_rng(21)
    acts = rng.uniform(-1, 1, (80, n)).astype(F32)
    s0 = np.stack([rng.uniform(-1.2, 0.6, n), rng.uniform(-0.07, 0.07, n)]).astype(F32)
    with gpu_pkg.VectorEnv(GYM, n, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=40) as a:
        a.Reset()
        a.SetState(s0)
        assert _eq(a.GetState(), s0) and _eq(a.Read().Observation, s0.T)
        for t in range(30):
            a.Step(acts[t])
        ck = a.Checkpoint()
        tail_a = [a.Step(acts[t]) for t in range(30, 80)]
        end_a = a.GetState()
    assert any(x.Done.any() for x in tail_a) and any(x.Truncated.any() for x in tail_a)
    with gpu_pkg.VectorEnv(GYM, n, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=40) as b:
        b.Reset()
        b.Restore(ck)
        tail_b = [b.Step(acts[t]) for t in range(30, 80)]
        assert _eq(b.GetState(), end_a)
    for x, y in zip(tail_a, tail_b):
        assert _eq(x.Observation, y.Observation) and _eq(x.Reward, y.Reward) and _eq(x.Done, y.Done) and _eq(x.Truncated, y.Truncated)


# ---- 7. groups -----------------------------------------------------------------------------------------------------------------
def test_group_of_two_members_equals_one_handle(gpu_pkg):
    G, n = 2, 2 * 1024
    nl = n // G
    rng = np.random.default_rng(7)
    s0 = np.stack([rng.uniform(-0.6, 0.5, n), rng.uniform(-0.02, 0.07, n)]).astype(F32)      # many lanes finish and reset
    with gpu_pkg.GroupVectorEnv(GYM, n, G, devices=[0] * G, seed=SEED, auto_reset=True, gather="direct") as grp, \
            gpu_pkg.VectorEnv(GYM, n, seed=SEED, auto_reset=True) as one:
        assert grp._adtype == np.float32 and grp.ObsDim == 2
        assert np.array_equal(grp.Reset(), one.Reset())
        one.SetState(s0)
        for m in range(G):
            grp.Members[m].SetState(s0[:, m * nl:(m + 1) * nl])
        finished = 0
        for t in range(12):
            a = rng.uniform(-1.5, 1.5, n).astype(F32)
            x, y = grp.Step(a), one.Step(a)
            assert _eq(x.Observation, y.Observation) and _eq(x.Reward, y.Reward) and _eq(x.Done, y.Done), t
            finished += int(y.Done.sum())
            grp.AllGatherObs(); grp.WaitGather(); grp.Sync()
            for m in range(G):
                assert _eq(np.concatenate(list(grp.ReadReplica(m)), axis=1).T, y.Observation), (t, m)
        assert finished > 0
