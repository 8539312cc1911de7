"""The edge-state tables of Pendulum, MountainCar and Acrobot (tests/_env_edge_tables.py) through every kernel form, on the GPU.

Each table is tiled into a batch sized by the rules of tests/_instantiation_matrix.py (a full workgroup, a partial last wave, n % V != 0
where the form allows it) and rotated from one repetition to the next, so that every row sits in every sub-lane position of a thread
and every non-finite row has finite rows next to it — on Acrobot's packed form, in the other half of its register pair.  One step
(two for the fused rollouts), with auto-reset off and on:
  - state, observation, reward and done equal the float32 twin bit for bit, NaN in the same places (so a finite row next to a NaN row
    is untouched, and with auto-reset a done row carries the oracle's reset draw while a NaN row — never done — is left as it is);
  - the hand-derived facts of the rows hold for what the kernel stored;
  - finite rows meet the float64 bars (T.check_float64_bars).
Pendulum angles beyond 65536 go through the device math library, which may differ from the host's by an ulp: there the state and the
observation are held to the float64 bars and to the library bound instead of the twin's bits; the reward, which has no trigonometry
in it, stays bit-identical.  On a bookkeeping handle a NaN lane is truncated at max_episode_steps like any other, and the fused reset
replaces it with a finite draw."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _env_edge_tables as T  # noqa: E402
import _instantiation_matrix as M  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
SEED = 0x5EED
SHORT = {"Pendulum-v1": "Pendulum", "MountainCar-v0": "MountainCar", "Acrobot-v1": "Acrobot"}
BLOCK = 256


def _eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- the tables, in an order that puts a finite row on both sides of every non-finite one ---------------------------------------------
def _spread(rows, s, a):
    fin = [i for i, r in enumerate(rows) if r["finite"]]
    bad = [i for i, r in enumerate(rows) if not r["finite"]]
    gap = len(fin) // (len(bad) + 1)
    assert gap >= 2
    order = []
    for k, i in enumerate(fin):
        order.append(i)
        if (k + 1) % gap == 0 and bad:
            order.append(bad.pop(0))
    assert not bad
    return [rows[i] for i in order], s[:, order].copy(), a[order].copy()


_TABLES = {}


def table(oracle, gym):
    """Rows, states and actions in spread order, with the float64 oracle's and the literal transcription's results per row."""
    if gym not in _TABLES:
        rows, s, a = _spread(*T.table_arrays(gym))
        s2, obs, rw, d = oracle.env_step(gym, s, a, dtype=np.float64)
        t = dict(rows=rows, s=s, a=a, f64=dict(s2=s2, obs=obs, reward=rw, done=d))
        if gym == "Acrobot-v1":
            t["literal"] = oracle.acrobot_step_f32_literal(s, a)[0]
        _TABLES[gym] = t
    return _TABLES[gym]


def tiling(R, n, v):
    """lane -> row for n lanes over R rows: repetition j starts c * j rows further on, with the smallest c that puts every row into
    every position i % v of a thread's lanes."""
    lane = np.arange(n)
    for c in range(1, 9):
        m = (lane % R + c * (lane // R)) % R
        if all(len(np.unique(m[lane % v == p])) == R for p in range(v)):
            return m
    raise AssertionError((R, n, v))


def batch(t, n, v):
    m = tiling(len(t["rows"]), n, v)
    rows = [t["rows"][i] for i in m]
    fin = np.array([r["finite"] for r in rows])
    # a non-finite row never sits between two non-finite ones, and in a thread of v lanes it has a finite partner somewhere in the batch
    bad = np.nonzero(~fin)[0]
    assert len(bad) and all(fin[max(i - 1, 0)] or fin[min(i + 1, n - 1)] for i in bad)
    if v == 2:
        for name in {rows[i]["name"] for i in bad}:
            assert any(fin[i ^ 1] for i in bad if rows[i]["name"] == name and (i ^ 1) < n), name
    f64 = {k: (x[:, m] if x.ndim == 2 else x[m]) for k, x in t["f64"].items()}
    return dict(m=m, rows=rows, s=t["s"][:, m].copy(), a=t["a"][m].copy(), fin=fin, upstream=np.array([r["upstream"] for r in rows]), f64=f64,
                literal=t["literal"][:, m] if "literal" in t else None)


# ---- expectations ---------------------------------------------------------------------------------------------------------------
def twin_step(oracle, gym, s, a, auto, tick, lane0=0):
    if auto:
        s2, obs, rw, d = oracle.env_autoreset_step(gym, SEED, lane0, tick, s, a)
    else:
        s2, obs, rw, d = oracle.env_step(gym, s, a, dtype=f32)
    return dict(s2=s2, obs=obs, reward=rw.astype(f32), done=d.astype(bool))


def library_lanes(gym, s, s2):
    """Pendulum lanes whose sin / cos went through the math library: the angle stepped from, or the angle observed, beyond 65536."""
    if gym != "Pendulum-v1":
        return np.zeros(s.shape[1], bool)
    with np.errstate(invalid="ignore"):
        return (np.abs(s[0]) > 65536.0) | (np.abs(s2[0]) > 65536.0)


def check_step(oracle, gym, b, got, auto, tick, lane0=0):
    """One step of batch b as the kernel stored it (got: s2 [S, n], obs [O, n], reward, done) against twin, facts and float64."""
    want = twin_step(oracle, gym, b["s"], b["a"], auto, tick, lane0)
    lib = library_lanes(gym, b["s"], want["s2"])
    assert _eq(got["reward"], want["reward"]) and _eq(got["done"], want["done"])
    assert _eq(got["s2"][:, ~lib], want["s2"][:, ~lib]) and _eq(got["obs"][:, ~lib], want["obs"][:, ~lib])
    assert np.isnan(want["s2"]).any() and np.isfinite(want["s2"][:, b["fin"] & b["upstream"]]).all()
    done = want["done"]
    assert (lib.sum() > 0) == (gym == "Pendulum-v1") and not (lib & done).any()
    # the facts, for what the kernel itself stored (a lane the fused reset replaced keeps only its flag and its reward)
    T.check_facts(b["rows"], got["s2"], got["reward"], got["done"], f32, "gpu", only=~done if auto else None)
    if auto and done.any():
        fs, fo = oracle.env_reset(gym, SEED, lane0, tick, len(done), with_obs=True)
        assert _eq(got["s2"][:, done], fs[:, done]) and _eq(got["obs"][:, done], fo[:, done]) and np.isfinite(fs).all()
        for i in np.nonzero(done)[0]:
            assert ("done", False) not in b["rows"][i]["facts"], b["rows"][i]["name"]
    nan_in = ~b["fin"] & np.isnan(want["s2"]).any(axis=0)
    assert nan_in.any() and not done[nan_in].any() and np.isnan(got["s2"][:, nan_in]).any(axis=0).all()      # a NaN lane is never done, never reset
    use = b["fin"] & b["upstream"] & (~done if auto else True)
    T.check_float64_bars(gym, b["s"], b["f64"], got, use, literal=b["literal"])
    if lib.any():                                                                   # beyond 65536: the library bound, from the stored angle
        fl = lib & b["fin"]
        own = got["s2"][0, fl].astype(np.float64)
        assert np.abs(got["obs"][0, fl] - np.cos(own)).max() <= T.LIBRARY_SINCOS_BOUND
        assert np.abs(got["obs"][1, fl] - np.sin(own)).max() <= T.LIBRARY_SINCOS_BOUND
        assert _eq(got["obs"][2, lib], got["s2"][1, lib])


# ---- one-launch step forms -----------------------------------------------------------------------------------------------------
def _step_forms():
    out = []
    for gym, env in SHORT.items():
        e = M.ENVS[env]
        for auto in (False, True):
            ar = "true" if auto else "false"
            for v in sorted({1, M.wide_of(env)}):
                launch = dict(vec=v, nt=15, block=BLOCK, sequential_lanes=1)
                if e["alias"]:
                    launch["reset_form"] = 0
                if env == "Acrobot":
                    launch["lds_pipe"] = 0
                out.append((gym, auto, f"step_kernel<{env},{v},{ar},false,15,0>", launch, M._one_shot_n(v, BLOCK), v))
            if env == "Acrobot":
                for items in (4, 5):
                    out.append((gym, auto, f"step_kernel_pipe<Acrobot,{items},{ar},15>", dict(vec=1, sequential_lanes=items, lds_pipe=0),
                                2 * 256 * items + 77, 1))
                out.append((gym, auto, f"step_kernel_lds<Acrobot,2,{ar},15>", dict(vec=1, sequential_lanes=2, lds_pipe=1), 5 * M.LDS_TILE, 1))
                out.append((gym, auto, f"step_kernel_pipe2<Acrobot,2,{ar},15>", dict(vec=2, sequential_lanes=2, block=BLOCK, nt=15, lds_pipe=0),
                            3 * (2 * 2 * 256), 2))
    return [pytest.param(*f, id=f[2]) for f in out]


@pytest.mark.parametrize("gym,auto,name,launch,n,v", _step_forms())
def test_step_forms_on_the_edge_tables(gpu_pkg, oracle, gym, auto, name, launch, n, v):
    b = batch(table(oracle, gym), n, v)
    with gpu_pkg.VectorEnv(gym, n, seed=SEED, auto_reset=auto, launch_policy=launch) as env:
        env.ResetDevice()
        env.SetState(b["s"])
        assert env.KernelName() == name
        assert _eq(env.GetState(), b["s"])
        tick = env.Tick
        out = env.Step(b["a"])
        got = dict(s2=env.GetState(), obs=out.Observation.T.copy(), reward=out.Reward, done=out.Done)
        assert env.KernelName() == name
    check_step(oracle, gym, b, got, auto, tick)


# ---- fused ring rollouts, two steps ----------------------------------------------------------------------------------------------
def _rollout_forms():
    out = []
    for gym, env in SHORT.items():
        for auto in (False, True):
            for v in (1, M.wide_of(env)):
                n = 2 * M.ROLLOUT_BLOCK + 103 if v == 1 else v * (2 * M.ROLLOUT_BLOCK + 100)
                launch = dict(vec=v)
                if M.ENVS[env]["alias"]:
                    launch["reset_form"] = 0
                name, got_v = M.rollout_instantiation(env, v, n, auto, False, "ring", False, False, 0, action_stride=n)
                assert got_v == v
                out.append((gym, auto, name, launch, n, v))
    return [pytest.param(*f, id=f[2]) for f in out]


@pytest.mark.parametrize("gym,auto,name,launch,n,v", _rollout_forms())
def test_fused_rollouts_on_the_edge_tables(gpu_pkg, oracle, gym, auto, name, launch, n, v):
    import torch
    b = batch(table(oracle, gym), n, v)
    a2 = np.roll(b["a"], 1)                                                        # the second step: every lane takes its neighbour's action
    with gpu_pkg.VectorEnv(gym, n, seed=SEED, auto_reset=auto, launch_policy=launch) as env:
        env.ResetDevice()
        env.SetState(b["s"])
        O = env.ObsDim
        ring = torch.from_numpy(np.stack([b["a"], a2])).cuda()
        rec_o = torch.zeros((2, O, n), dtype=torch.float32, device="cuda")
        rec_r = torch.zeros((2, n), dtype=torch.float32, device="cuda")
        rec_d = torch.zeros((2, n), dtype=torch.uint8, device="cuda")
        assert all(x.data_ptr() % 16 == 0 for x in (ring, rec_o, rec_r, rec_d)) and n % v == 0 and ring.stride(0) % v == 0
        pol = env.GetLaunchPolicy()
        assert M.rollout_instantiation(SHORT[gym], pol["vec"], n, auto, False, "ring", False, False, pol["reset_form"], action_stride=n) == (name, v)
        tick = env.Tick
        torch.cuda.synchronize()
        env.RolloutFusedDevice(ring, 2, n, 2, rec_obs=rec_o, rec_reward=rec_r, rec_done=rec_d)
        env.Sync()
        assert env.Tick == tick + 2
        go, gr, gd, final = rec_o.cpu().numpy(), rec_r.cpu().numpy(), rec_d.cpu().numpy().astype(bool), env.GetState()
    w1 = twin_step(oracle, gym, b["s"], b["a"], auto, tick)
    w2 = twin_step(oracle, gym, w1["s2"], a2, auto, tick + 1)
    lib = library_lanes(gym, b["s"], w1["s2"]) | library_lanes(gym, w1["s2"], w2["s2"])
    assert _eq(gr[0], w1["reward"]) and _eq(gd[0], w1["done"]) and _eq(go[0][:, ~lib], w1["obs"][:, ~lib])
    assert _eq(gr[1][~lib], w2["reward"][~lib]) and _eq(gd[1], w2["done"]) and _eq(go[1][:, ~lib], w2["obs"][:, ~lib])
    assert _eq(final[:, ~lib], w2["s2"][:, ~lib])
    assert np.isnan(final).any() and (gym == "Pendulum-v1" or w1["done"].any())
    # the first step's flags and rewards against the facts that speak of them, and its observation against float64
    rows = b["rows"]
    for i in range(n):
        for f in rows[i]["facts"]:
            if f[0] == "done":
                assert gd[0][i] == f[1], rows[i]["name"]
            elif f[0] == "reward":
                assert gr[0][i] == f32(f[1]), rows[i]["name"]
    use = b["fin"] & b["upstream"] & ~w1["done"]
    if gym == "MountainCar-v0":
        assert np.abs(go[0][:, use].astype(np.float64) - b["f64"]["obs"][:, use]).max() <= 1e-6
    if lib.any():
        fl = lib & b["fin"] & np.isfinite(final).all(axis=0)
        own = final[0, fl].astype(np.float64)
        assert np.abs(go[1][0, fl] - np.cos(own)).max() <= T.LIBRARY_SINCOS_BOUND and np.abs(go[1][1, fl] - np.sin(own)).max() <= T.LIBRARY_SINCOS_BOUND
        assert np.abs(final[1, fl].astype(np.float64) - w2["s2"][1, fl]).max() <= 1e-5


# ---- the resident kernel: at most 64 lanes, so the table goes through in slices ---------------------------------------------------
@pytest.mark.parametrize("auto", [False, True], ids=["keep", "autoreset"])
@pytest.mark.parametrize("gym", sorted(SHORT))
def test_resident_kernel_on_the_edge_tables(gpu_pkg, oracle, gym, auto):
    t = table(oracle, gym)
    R = len(t["rows"])
    whole = batch(t, R, 1)                                                          # every row once, in spread order
    got = dict(s2=np.zeros_like(whole["s"]), obs=None, reward=np.zeros(R, f32), done=np.zeros(R, bool))
    ticks = set()
    for lo in range(0, R, 64):
        hi = min(lo + 64, R)
        # (lane_offset: the slice's rows keep the global lanes, and with them the reset draws, of the whole table)
        with gpu_pkg.VectorEnv(gym, hi - lo, seed=SEED, auto_reset=auto, resident=True, lane_offset=lo) as env:
            env.Reset()
            env.SetState(whole["s"][:, lo:hi])
            ticks.add(env.Tick)
            out = env.Step(whole["a"][lo:hi])
            if got["obs"] is None:
                got["obs"] = np.zeros((env.ObsDim, R), f32)
            got["s2"][:, lo:hi], got["obs"][:, lo:hi] = env.GetState(), out.Observation.T
            got["reward"][lo:hi], got["done"][lo:hi] = out.Reward, out.Done
    assert len(ticks) == 1
    check_step(oracle, gym, whole, got, auto, ticks.pop())


# ---- a NaN lane on a bookkeeping handle: truncated at the limit, replaced by a finite draw -----------------------------------------
@pytest.mark.parametrize("gym", sorted(SHORT))
def test_nan_lanes_are_truncated_at_the_limit_and_reset(gpu_pkg, oracle, gym):
    limit, n = 11, M._one_shot_n(1, BLOCK)
    b = batch(table(oracle, gym), n, 1)
    launch = dict(vec=1, nt=15, block=BLOCK, sequential_lanes=1)
    if M.ENVS[SHORT[gym]]["alias"]:
        launch["reset_form"] = 0
    if gym == "Acrobot-v1":
        launch["lds_pipe"] = 0
    with gpu_pkg.VectorEnv(gym, n, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=limit, launch_policy=launch) as env:
        env.ResetDevice()
        env.SetState(b["s"])
        assert env.KernelName() == f"step_kernel<{SHORT[gym]},1,true,true,15,0>"
        ln = np.where(np.arange(n) % 2 == 0, limit - 1, 3).astype(np.int32)           # every other lane reaches the limit with this step
        env.SetArray("episode_length", ln)
        env.SetArray("episode_return", np.zeros(n, f32))
        tick = env.Tick
        out = env.Step(b["a"])
        got_s, got_d = env.GetState(), env.GetArray("done")
    want = twin_step(oracle, gym, b["s"], b["a"], False, tick)
    fs, fo = oracle.env_reset(gym, SEED, 0, tick, n, with_obs=True)
    trunc = ln + 1 >= limit
    byte = want["done"].astype(np.uint8) | np.where(trunc, 2, 0).astype(np.uint8)
    fin = byte != 0
    lib = library_lanes(gym, b["s"], want["s2"])
    nan_lane = np.isnan(want["s2"]).any(axis=0)
    assert (nan_lane & trunc).any() and (nan_lane & ~trunc).any()
    assert _eq(got_d, byte) and _eq(out.Reward, want["reward"]) and _eq(out.Truncated, trunc)
    assert _eq(got_s[:, fin], fs[:, fin]) and _eq(out.Observation.T[:, fin], fo[:, fin])
    assert np.isfinite(got_s[:, nan_lane & trunc]).all()                             # the poisoned lane is gone
    assert np.isnan(got_s[:, nan_lane & ~trunc]).any(axis=0).all()                   # ... and before the limit it is left as it is
    keep = ~fin & ~lib
    assert _eq(got_s[:, keep], want["s2"][:, keep]) and _eq(out.Observation.T[:, keep], want["obs"][:, keep])
