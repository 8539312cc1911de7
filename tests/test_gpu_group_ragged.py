"""GPU tests of gymnet_group_* at ragged member sizes (tests/_group_ragged_cases.py holds the table and what each size reaches):
a GroupVectorEnv of G logical members on device 0 beside ONE VectorEnv over the same global lanes, same seed, auto-reset on.
Every comparison is bitwise, floats through uint32 / uint64 views (NaN payloads and signed zeros would count).

Per row of the table:
  - test_host_boundary: Reset() and 8 Step(a) of the group equal the single handle's in observation, reward, done and truncated —
    group_copy_out()'s host-mapped export for members of <= 4096 lanes, pack + memcpy above, both with a row stride of n_local;
  - test_device_path: ResetDevice, then 11 x (StepDevice with per-member slices of ONE action tensor — slices that start 4, 8 or 12
    bytes off a 16-byte line — then AllGatherObs); with overlap every other gather stays in flight across the next step.  At every
    checked step EVERY member's replica [G][D][n_local] equals the single handle's observation (ReadReplica and a zero-copy view
    of GlobalObsPtr, which must follow the buffer gathered last), every member's observation / reward / done equal its slice, and
    every member's tick equals the single handle's;
  - the form each member resolved to, from KernelName() and LaunchPolicy(): one lane per thread wherever a row of the member is off
    the wide form's line, with SetLaunchPolicy(vec = wide) refused and the kernel unchanged; the wide form where forced (two rows)
    or where float64 rows allow it.  test_case_table_reaches_wide_forms_and_fallbacks fails if the table loses either kind.
A few lanes per member start one step from a terminal state (Pendulum, which has none, runs under a time limit), so every run
re-draws lanes through the fused reset, whose Philox lane groups straddle the member boundaries at these sizes.

The group entry points nobody else calls, at CartPole 3 x 1001 and Pendulum 3 x 1002: test_group_seed (gymnet_group_seed, twice),
test_group_time_limit (the group's max_episode_steps with episode statistics), test_group_validation_at_a_ragged_size (one bad
action in the last member's last lane: staged action slices that are not 16-byte aligned).

test_group_rollout_with_an_odd_ring: rollout_steps()' odd-ring rule (a captured graph of 2 * ring steps, so that tick slot,
done-count half and observation buffer return to where they were) on the group's path — ring 5, action stride != lanes, 23 steps
= two replays + three eager steps, twice, against an EAGER single-handle rollout.

Each case runs in about a second or less.
"""
import numpy as np
import pytest

from _group_ragged_cases import CASES, F64, KERNEL_ENV, TIME_LIMIT, case_id, expected_vec, rows_allow, wide_form

gpu = pytest.mark.gpu
SEED = 0x5EED
NACT = {"CartPole-v1": 2, "MountainCar-v0": 3, "Acrobot-v1": 3}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _actions(rng, name, n):
    """random actions; Box envs also get values outside their bounds (the kernels clip: Pendulum to [-2, 2], MountainCarContinuous to [-1, 1])"""
    if name in NACT:
        return rng.integers(0, NACT[name], n).astype(np.int32)
    return rng.uniform(-3, 3, n).astype(np.float32)


def _start_state(name, dtype, base):
    """`base` [S, n] (the state after a reset) with every third lane moved one step from a terminal state, so that lanes finish —
    and are re-drawn by the fused reset — within the first steps whatever the batch size"""
    s = base.copy()
    lanes = np.arange(s.shape[1]) % 3 == 0
    if name == "CartPole-v1":
        s[0, lanes], s[1, lanes] = 2.39, 2.0                 # x + 0.02 * x_dot > 2.4
    elif name == "MountainCar-v0":
        s[0, lanes], s[1, lanes] = 0.495, 0.07               # position >= 0.5 with velocity >= 0
    elif name == "MountainCarContinuous-v0":
        s[0, lanes], s[1, lanes] = 0.449, 0.07               # position >= 0.45
    elif name == "Acrobot-v1":
        s[:, lanes] = np.array([np.pi, 0.0, 0.0, 0.0], dtype)[:, None]      # upright: -cos(t1) - cos(t1 + t2) = 2 > 1
    return s.astype(dtype)


def _force_finishing_lanes(name, dtype, grp, one):
    if name in TIME_LIMIT:
        return
    nl = grp.LanesPerMember
    s = _start_state(name, dtype, one.GetState())
    one.SetState(s)
    for m, mem in enumerate(grp.Members):
        mem.SetState(s[:, m * nl:(m + 1) * nl])


def _open(gpu_pkg, case, **kw):
    env, dtype, G, nl, overlap, force = case
    limit = TIME_LIMIT.get(env, 0)
    common = dict(seed=SEED, auto_reset=True, max_episode_steps=limit, episode_stats=bool(limit), dtype=dtype, **kw)
    grp = gpu_pkg.GroupVectorEnv(env, G * nl, G, devices=[0] * G, gather="direct", overlap=overlap, **common)
    one = gpu_pkg.VectorEnv(env, G * nl, **common)
    return grp, one


def _check_forms(case, grp):
    """every member resolved to the expected lanes per thread; a wide form its rows do not allow is refused and changes nothing"""
    env, dtype, G, nl, overlap, force = case
    wide, want = wide_form(env, dtype), expected_vec(case)
    family = f"step_kernel<{KERNEL_ENV[env]}{'64' if dtype is F64 else ''},"
    extras = "true" if env in TIME_LIMIT else "false"
    for m, mem in enumerate(grp.Members):
        if force:
            mem.SetLaunchPolicy(vec=force)
        name = mem.KernelName()
        assert name.startswith(f"{family}{want},true,{extras},"), (m, name)
        assert mem.LaunchPolicy()["envs_per_thread"] == want, (m, mem.LaunchPolicy())
        if not rows_allow(env, dtype, G, nl, wide):
            assert want == 1
            with pytest.raises(ValueError):
                mem.SetLaunchPolicy(vec=wide)
            assert mem.KernelName() == name and mem.LaunchPolicy()["envs_per_thread"] == 1
        if env == "Acrobot-v1":
            with pytest.raises(ValueError):
                mem.SetLaunchPolicy(vec=4)                 # Acrobot has no four-lane form
            assert mem.KernelName() == name


def test_case_table_reaches_wide_forms_and_fallbacks():
    forms = {(wide_form(c[0], c[1]), expected_vec(c)) for c in CASES}
    assert {(4, 4), (2, 2)} <= forms, "no row runs a wide form"
    assert {(4, 1), (2, 1)} <= forms, "no row runs the one-lane fallback"
    assert any(c[1] is F64 and expected_vec(c) == 2 and not c[5] for c in CASES) and any(c[1] is F64 and expected_vec(c) == 1 for c in CASES)
    assert {c[3] % 4 for c in CASES} == {0, 1, 2, 3} and {c[3] > 4096 for c in CASES} == {False, True}
    assert {(m * c[3]) % 4 for c in CASES for m in range(c[2])} == {0, 1, 2, 3}         # a member's first global lane, mod 4
    assert max(c[2] for c in CASES) == 16 and len(CASES) <= 20 and len({case_id(c) for c in CASES}) == len(CASES)


@gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_host_boundary(gpu_pkg, case):
    env, dtype, G, nl, overlap, force = case
    n = G * nl
    rng = np.random.default_rng(nl)
    grp, one = _open(gpu_pkg, case)
    with grp, one:
        assert grp.LanesPerMember == nl and len(grp.Members) == G
        _check_forms(case, grp)
        assert _same(grp.Reset(), one.Reset())
        _force_finishing_lanes(env, dtype, grp, one)
        finished = 0
        for t in range(8):
            a = _actions(rng, env, n)
            g, o = grp.Step(a), one.Step(a)
            assert _same(g.Observation, o.Observation), t
            assert _same(g.Reward, o.Reward) and np.array_equal(g.Done, o.Done) and np.array_equal(g.Truncated, o.Truncated), t
            finished += int(o.Done.sum())
            if env in TIME_LIMIT:
                assert o.Truncated.all() == ((t + 1) % TIME_LIMIT[env] == 0) and o.Truncated.any() == o.Truncated.all()
        assert finished > 0, "no lane finished: the fused reset never ran"
        assert [m.Tick for m in grp.Members] == [one.Tick] * G


def _global_obs_view(torch, grp, member, dtype, shape):
    """zero-copy torch view of gymnet_group_global_obs(member), the way sharding.py views a peer buffer"""
    class _Raw:
        __cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f8" if dtype is F64 else "<f4",
                                    "data": (grp.GlobalObsPtr(member), False), "version": 2}
    return torch.as_tensor(_Raw(), device=torch.device("cuda", 0))


def _check_gather(torch, case, grp, one, want, tag, seen_ptrs):
    """every member's replica (host copy and zero-copy view), observation / reward / done slices and tick against the single handle"""
    env, dtype, G, nl, overlap, force = case
    D = want.Observation.shape[1]
    whole = np.ascontiguousarray(want.Observation.T)                                   # [D, n]
    want_rep = np.stack([whole[:, m * nl:(m + 1) * nl] for m in range(G)])             # [G, D, nl]
    for m in range(G):
        rep = grp.ReadReplica(m)
        assert _same(rep, want_rep), (tag, "replica of member", m, np.argwhere(_bits(rep) != _bits(want_rep))[:3].tolist())
        seen_ptrs[m].add(grp.GlobalObsPtr(m))
        view = _global_obs_view(torch, grp, m, dtype, (G, D, nl)).cpu().numpy()
        assert _same(view, rep), (tag, "GlobalObsPtr of member", m)
        r = grp.Members[m].Read()
        sl = slice(m * nl, (m + 1) * nl)
        assert _same(r.Observation, want.Observation[sl]), (tag, m)
        assert _same(r.Reward, want.Reward[sl]) and np.array_equal(r.Done, want.Done[sl]) and np.array_equal(r.Truncated, want.Truncated[sl]), (tag, m)
        assert grp.Members[m].Tick == one.Tick, (tag, m)


@gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_device_path(gpu_pkg, case):
    import torch
    env, dtype, G, nl, overlap, force = case
    n, steps = G * nl, 11
    rng = np.random.default_rng(7 * nl + G)
    grp, one = _open(gpu_pkg, case)
    with grp, one:
        _check_forms(case, grp)
        grp.ResetDevice(); one.Reset()
        _force_finishing_lanes(env, dtype, grp, one)
        seen_ptrs = [set() for _ in range(G)]
        grp.AllGatherObs(); grp.WaitGather(); grp.Sync()
        _check_gather(torch, case, grp, one, one.Read(), "reset", seen_ptrs)
        acts = torch.empty(n, dtype=torch.int32 if env in NACT else torch.float32, device="cuda")
        assert acts.data_ptr() % 16 == 0
        finished = 0
        for t in range(steps):
            a = _actions(rng, env, n)
            acts.copy_(torch.from_numpy(a)); torch.cuda.synchronize()
            grp.StepDevice([acts[m * nl:(m + 1) * nl] for m in range(G)])
            grp.AllGatherObs()
            out = one.Step(a)
            finished += int(out.Done.sum())
            if overlap and t % 2 == 0 and t + 1 < steps:
                continue                                   # this gather stays in flight across the next step
            grp.WaitGather(); grp.Sync()
            _check_gather(torch, case, grp, one, out, t, seen_ptrs)
        assert finished > 0, "no lane finished: the fused reset never ran"
        # steps 1, 3, .., 9 leave the latest observation in buffer 0, step 10 in buffer 1: GlobalObsPtr follows the buffer gathered last
        assert all(len(p) == (2 if overlap else 1) for p in seen_ptrs), seen_ptrs
        assert len(set().union(*seen_ptrs)) == G * (2 if overlap else 1)


RAGGED_PAIR = [("CartPole-v1", 1001), ("Pendulum-v1", 1002)]


@gpu
@pytest.mark.parametrize("env,nl", RAGGED_PAIR)
def test_group_seed(gpu_pkg, env, nl):
    G = 3
    n = G * nl
    rng = np.random.default_rng(11)
    with gpu_pkg.GroupVectorEnv(env, n, G, devices=[0] * G, seed=1, auto_reset=True, gather="direct", overlap=True) as grp, \
            gpu_pkg.VectorEnv(env, n, seed=1, auto_reset=True) as one:
        first = None
        for seed in (0xC0FFEE, 0x5EED0000BEEF, 0xC0FFEE):          # the second and third Seed() land mid-run
            grp.Seed(seed); one.Seed(seed)
            assert [m.GetSeed() for m in grp.Members] == [one.GetSeed()] * G == [(seed, False)] * G
            assert [m.Tick for m in grp.Members] == [one.Tick] * G == [0] * G
            g0, o0 = grp.Reset(), one.Reset()
            assert _same(g0, o0)
            if first is None:
                first = o0
            elif seed == 0xC0FFEE:
                assert _same(o0, first)                             # the same seed draws the same batch again
            else:
                assert not _same(o0, first)
            _force_finishing_lanes(env, np.float32, grp, one)
            finished = 0
            for t in range(5):
                a = _actions(rng, env, n)
                g, o = grp.Step(a), one.Step(a)
                assert _same(g.Observation, o.Observation) and _same(g.Reward, o.Reward) and np.array_equal(g.Done, o.Done), (seed, t)
                finished += int(o.Done.sum())
            assert finished > 0 or env not in NACT                  # (Pendulum has no terminal state and this test no time limit)
            grp.AllGatherObs(); grp.WaitGather(); grp.Sync()
            for m in range(G):
                assert _same(np.concatenate(list(grp.ReadReplica(m)), axis=1).T, o.Observation), (seed, m)


@gpu
@pytest.mark.parametrize("env,nl", RAGGED_PAIR)
def test_group_time_limit(gpu_pkg, env, nl):
    G, limit = 3, 7
    n = G * nl
    rng = np.random.default_rng(13)
    kw = dict(seed=SEED, auto_reset=True, max_episode_steps=limit, episode_stats=True)
    with gpu_pkg.GroupVectorEnv(env, n, G, devices=[0] * G, gather="direct", **kw) as grp, gpu_pkg.VectorEnv(env, n, **kw) as one:
        assert _same(grp.Reset(), one.Reset())
        truncated_at = []
        for t in range(2 * limit + 2):
            a = _actions(rng, env, n)
            g, o = grp.Step(a), one.Step(a)
            assert np.array_equal(g.Truncated, o.Truncated) and np.array_equal(g.Done, o.Done), t
            assert _same(g.Observation, o.Observation) and _same(g.Reward, o.Reward), t
            assert not (o.Truncated & ~o.Done).any()                 # a truncated lane is a finished lane
            if o.Truncated.any():
                truncated_at.append(t)
            ret, ln = one.EpisodeStats()
            for m in range(G):
                r, l = grp.Members[m].EpisodeStats()
                assert _same(r, ret[m * nl:(m + 1) * nl]) and np.array_equal(l, ln[m * nl:(m + 1) * nl]), (t, m)
            longest = int(ln.max())                                  # finished lengths: none outlives the limit, and from step `limit` on one reaches it
            assert longest == limit if t + 1 >= limit else longest <= t + 1, (t, longest)
        assert truncated_at[0] == limit - 1 and 2 * limit - 1 in truncated_at
        assert int(one.EpisodeStats()[1].max()) == limit             # the largest finished length is the limit
        if env == "Pendulum-v1":                                     # no terminal state: every lane is truncated together, and only then
            assert truncated_at == [limit - 1, 2 * limit - 1]


@gpu
def test_group_validation_at_a_ragged_size(gpu_pkg):
    """One bad action in the LAST member's LAST lane rejects the step before any member has advanced, host and device form; the
    members' action slices start 4004 and 8008 bytes into the batch.  (Box actions are clipped, never refused: CartPole only.)"""
    import torch
    G, nl = 3, 1001
    n = G * nl
    rng = np.random.default_rng(17)
    with gpu_pkg.GroupVectorEnv("CartPole-v1", n, G, devices=[0] * G, seed=SEED, auto_reset=True, gather="direct", validate_actions=True) as grp, \
            gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True) as one:
        assert _same(grp.Reset(), one.Reset())
        ticks = [m.Tick for m in grp.Members]
        a = rng.integers(0, 2, n).astype(np.int32)
        a[n - 1] = 2
        with pytest.raises(gpu_pkg.InvalidActionError):
            grp.Step(a)
        assert [m.Tick for m in grp.Members] == ticks
        da = torch.from_numpy(a).cuda(); torch.cuda.synchronize()
        with pytest.raises(gpu_pkg.InvalidActionError):
            grp.StepDevice([da[m * nl:(m + 1) * nl] for m in range(G)])
        assert [m.Tick for m in grp.Members] == ticks
        a[n - 1] = 1                                                  # nothing moved: the valid step equals the single handle's first step
        g, o = grp.Step(a), one.Step(a)
        assert _same(g.Observation, o.Observation) and np.array_equal(g.Done, o.Done)
        assert [m.Tick for m in grp.Members] == [t + 1 for t in ticks]
        da.copy_(torch.from_numpy(a)); torch.cuda.synchronize()
        grp.StepDevice([da[m * nl:(m + 1) * nl] for m in range(G)]); grp.Sync()
        o = one.Step(a)
        for m in range(G):
            assert _same(grp.Members[m].Read().Observation, o.Observation[m * nl:(m + 1) * nl])


@gpu
def test_group_rollout_with_an_odd_ring(gpu_pkg):
    import torch
    G, nl, ring, steps = 3, 1001, 5, 23                      # 23 = two replays of the 10-step graph + three eager steps
    n, stride = G * nl, nl + 3
    with gpu_pkg.GroupVectorEnv("CartPole-v1", n, G, devices=[0] * G, seed=SEED, auto_reset=True, gather="direct", overlap=True) as grp, \
            gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True, launch_policy={"graph": 0}) as one:    # eager: one launch per step
        acts = torch.empty((ring, n), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for t in range(ring):
            one.SampleActionsDevice(acts[t], seed=8, tick=t)
        one.Sync()
        macts = []
        for m in range(G):                                   # [ring][nl + 3] per member: the row stride is not the lane count
            buf = torch.full((ring, stride), 7, dtype=torch.int32, device="cuda")      # 7: no action, never read
            buf[:, :nl] = acts[:, m * nl:(m + 1) * nl]
            macts.append(buf)
        torch.cuda.synchronize()
        one.ResetDevice(); grp.ResetDevice()
        total = 1
        for call in range(3):                                # 23 is odd: the second call starts from the other parity, the third from the first again
            one.RolloutDevice(acts, steps, n, ring)
            grp.RolloutDevice(macts, steps, stride, ring)
            grp.AllGatherObs(); grp.WaitGather(); grp.Sync(); one.Sync()
            total += steps
            want = one.Read()
            assert want.Done.any() and one.Tick == total
            for m in range(G):
                rep = grp.ReadReplica(m)
                assert _same(np.concatenate(list(rep), axis=1).T, want.Observation), (call, m)
                r = grp.Members[m].Read()
                sl = slice(m * nl, (m + 1) * nl)
                assert _same(r.Reward, want.Reward[sl]) and np.array_equal(r.Done, want.Done[sl]), (call, m)
                assert grp.Members[m].Tick == one.Tick and grp.Members[m].Counters()["tick"] == one.Tick, (call, m)
                assert _same(grp.Members[m].GetState(), one.GetState()[:, sl]), (call, m)
