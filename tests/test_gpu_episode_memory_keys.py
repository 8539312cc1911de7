"""GPU checks of the episode memory's key order (gym.net_amd/csrc/episode_memory.hip, episode_memory_key.hpp) on the adversarial scripts
of tests/_episode_memory_cases.py: returns at the sign fold, keys that differ in one digit, ties decided by tick and lane, NaN returns,
capacity edges, K = 65536, a threshold that goes stale inside an ingest pass, and equal keys.  Every script goes through both entry points
on handles with the same seed and actions:
  single pushes   StepDevice, Sync, SetArray("reward", row), mem.Push(actions, done=row) — the handle keeps no episode statistics, so
                  nothing else reads the reward array;
  ingest          one RolloutFusedDevice of the segment's T steps recording observations, rewards and done bytes, Sync, the recorded
                  reward and done tensors overwritten with the script's rows, then mem.PushRollout, with rollout_chunk 1, 3 and 16.
After every push (single) or pass (ingest) Stats(), Episodes() and DatasetSize() are held to the model fed with the observations and
actions the device produced: returns as bit patterns with zero canonicalised, lengths, uint64 ticks, lanes.  At the end of a script the
params dataset is compared bit for bit, crafted rewards included, with the model's and between the two entry points.  Where equal keys
carry different rows (the tick set backwards) the device may keep either, so there the dataset's episodes are identified by the marker in
their first reward: each kept entry appears once, in listing order, with its own rows."""
import numpy as np
import pytest

import _episode_memory_cases as cases
import _episode_memory_model as model

pytestmark = pytest.mark.gpu
SEED = 0x5EED
SCRIPTS = {s["name"]: s for s in cases.scripts()}
# the largest capacity the memory takes, more lanes than that ending in one push (docs/ledger.md §40 has the times of this and of K = 16384)
LARGE_K, LARGE_N = 65536, 66001


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _obs_rows(env):
    """the handle's current observations, [N, D] on the host"""
    import torch
    rows = torch.empty((env.NumberOfEnvironments, env.ObsDim), dtype=getattr(torch, env.Dtype.name), device="cuda")
    env.PackObsDevice(rows)
    env.Sync()
    return rows.cpu().numpy()


def _actions(env, seed, rows):
    rng = np.random.default_rng(1000 + seed)
    n = env.NumberOfEnvironments
    if env._adtype == np.float32:
        return rng.uniform(env._info.action_low, env._info.action_high, (rows, n)).astype(np.float32)
    return rng.integers(0, env.ActionSpace.N, (rows, n)).astype(np.int32)


def _canon(ret):
    """float32 returns as bit patterns, -0 as +0"""
    r = np.array(ret, np.float32)
    r[r == 0] = 0.0
    return r.view(np.uint32)


def _observe(mem):
    return dict(stats=mem.Stats(), episodes=mem.Episodes(), rows=mem.DatasetSize())


def _dataset(mem):
    if mem.DatasetSize() == 0:
        return None
    return [None if v is None else v.cpu().numpy() for v in mem.BuildDataset("params", min_episodes=0, reward=True)]


def _run(pkg, s, chunk, ingest):
    """One handle through script s.  Returns the feed for the model (per segment: observations at its start [N, D], actions [T][N],
    observations after each step [T][N, D]), what the memory showed after every push (single) or pass (ingest) as (segment, step, dict),
    and the params dataset at the end."""
    import torch
    n = s["n"]
    with pkg.VectorEnv(s["env"], n, seed=SEED, auto_reset=True, dtype=getattr(np, s["dtype"])) as env:
        env.Reset()
        ck = mem = None
        feed, seen = [], []
        for i, seg in enumerate(s["segments"]):
            steps = seg["reward"].shape[0]
            if seg["restore"]:
                env.Restore(ck)
            elif env.Tick != seg["tick"]:
                env.Tick = seg["tick"]
            assert env.Tick == seg["tick"]
            if seg["checkpoint"]:
                ck = env.Checkpoint()
            if mem is None:
                mem = env.EpisodeMemory(capacity=s["capacity"], max_length=s["max_length"], history=s["history"], rollout_chunk=chunk)
            else:
                mem.Reset()
            obs0 = _obs_rows(env)
            acts = _actions(env, seg["action_seed"], steps)
            stride = (n + 63) // 64 * 64                                   # every action row 8-byte aligned, whatever n is
            d_acts = _dev(np.pad(acts, ((0, 0), (0, stride - n))))
            if ingest:
                obs = torch.empty((steps, env.ObsDim, n), dtype=getattr(torch, env.Dtype.name), device="cuda")
                rew = torch.empty((steps, n), dtype=torch.float32, device="cuda")
                done = torch.empty((steps, n), dtype=torch.uint8, device="cuda")
                env.RolloutFusedDevice(d_acts, steps, stride, steps, rec_obs=obs, rec_reward=rew, rec_done=done)
                env.Sync()
                rew.view(torch.int32).copy_(torch.from_numpy(seg["reward"].view(np.int32)))     # as integers: the bit patterns, untouched
                done.copy_(torch.from_numpy(seg["done"]))
                torch.cuda.synchronize()
                mem.PushRollout(steps, obs, d_acts, rew, done, action_stride=stride, ring=steps)
                env.Sync()
                rec = obs.cpu().numpy()
                after = [rec[t].T.copy() for t in range(steps)]
                seen.append((i, steps - 1, _observe(mem)))
            else:
                d_done = _dev(seg["done"])
                rows = seg["reward"].view(np.float32)
                after = []
                for t in range(steps):
                    env.StepDevice(d_acts[t])
                    env.Sync()
                    after.append(_obs_rows(env))
                    env.SetArray("reward", rows[t])
                    mem.Push(d_acts[t], done=d_done[t])
                    seen.append((i, t, _observe(mem)))
            assert env.Tick == seg["tick"] + steps
            feed.append((obs0, acts, after))
        return feed, seen, _dataset(mem)


def _check_against_model(s, trace, seen, what):
    by_push = {(rec["segment"], rec["step"]): rec for rec in trace}
    for segment, step, got in seen:
        rec = by_push[(segment, step)]
        where = (s["name"], what, segment, step)
        assert got["stats"] == rec["stats"], (where, got["stats"], rec["stats"])
        pool = sorted(rec["pool"], key=model.key, reverse=True)
        ret, length, tick, lane = got["episodes"]
        assert ret.dtype == np.float32 and tick.dtype == np.uint64 and not np.isnan(ret).any(), where
        assert np.array_equal(_canon(ret), _canon([e["ret"] for e in pool])), (where, ret)
        assert np.array_equal(length, np.array([e["len"] for e in pool], np.int32)), where
        assert np.array_equal(tick, np.array([e["tick"] for e in pool], np.uint64)), (where, tick)
        assert np.array_equal(lane, np.array([e["lane"] for e in pool], np.int32)), (where, lane)
        assert got["rows"] == sum(e["len"] * 2 // 3 for e in pool), where


def _same_bits(a, b, what):
    assert (a is None) == (b is None), what
    if a is None:
        return
    for x, y, name in zip(a, b, ("x", "action", "onehot", "reward")):
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), (what, name)


def _model_dataset(s, m):
    """the model's params dataset in the device's dtypes (None when it has no row)"""
    box = s["env"] == "Pendulum-v1"
    x, a, onehot, r = m.dataset_params(None if box else 2)
    if len(x) == 0:
        return None
    return [x, a.astype(np.float32 if box else np.int32), onehot, r]


def _check_marked_dataset(s, m, trace, got, data, what):
    """equal keys with different rows: every listed entry appears once in the dataset, in listing order, with the rows of ITS episode"""
    x, action, _, reward = data
    episodes = {int(m.rew[e["start"]][e["lane"]]): e for rec in trace for e in rec["ended"]}
    assert len(episodes) == len(s["markers"])
    ret, length, tick, lane = got["episodes"]
    off, used = 0, set()
    for i in range(len(ret)):
        rows = int(length[i]) * 2 // 3
        marker = int(reward[off])
        assert marker in s["markers"] and marker not in used, (what, i, marker)
        used.add(marker)
        assert (float(ret[i]), int(tick[i]), int(lane[i]), int(length[i])) == s["markers"][marker], (what, i, marker)
        e = episodes[marker]
        for p in range(rows):
            hist = [e["start"] + max(p - (m.history - 1) + q, 0) for q in range(m.history)]
            want = np.concatenate([m.obs[h][e["lane"]] for h in hist]).astype(np.float32)
            assert np.array_equal(x[off + p].view(np.uint32), want.view(np.uint32)), (what, i, p)
            assert int(action[off + p]) == int(m.act[e["start"] + p][e["lane"]]), (what, i, p)
            assert reward[off + p].view(np.uint32) == m.rew[e["start"] + p][e["lane"]].view(np.uint32), (what, i, p)
        off += rows
    assert off == len(reward), what


def _hold(pkg, s):
    feed, seen, data = _run(pkg, s, 0, ingest=False)
    assert len(seen) == sum(seg["reward"].shape[0] for seg in s["segments"])
    m, trace = cases.model_trace(s, feed)
    _check_against_model(s, trace, seen, "single pushes")
    marked = s["equal_keys"] == "backwards"
    if marked:
        _check_marked_dataset(s, m, trace, seen[-1][2], data, "single pushes")
    else:
        _same_bits(data, _model_dataset(s, m), "single pushes against the model")
    if s["equal_keys"] == "replay":                                        # the replayed segment saw what the first one saw
        (o0, a0, after0), (o1, a1, after1) = feed[0], feed[1]
        assert np.array_equal(o0, o1) and np.array_equal(a0, a1) and all(np.array_equal(p, q) for p, q in zip(after0, after1))
    for chunk in s["chunks"]:
        what = f"ingest, rollout_chunk {chunk}"
        feed_b, seen_b, data_b = _run(pkg, s, chunk, ingest=True)
        for (o0, a0, after0), (o1, a1, after1) in zip(feed, feed_b):       # the same env run: the model's feed holds for both
            assert np.array_equal(o0, o1) and np.array_equal(a0, a1) and all(np.array_equal(p, q) for p, q in zip(after0, after1)), what
        _check_against_model(s, trace, seen_b, what)
        assert seen_b[-1][2]["stats"] == seen[-1][2]["stats"], what
        for p, q in zip(seen_b[-1][2]["episodes"], seen[-1][2]["episodes"]):
            assert np.array_equal(p.view(np.uint8), q.view(np.uint8)), what
        if marked:
            _check_marked_dataset(s, m, trace, seen_b[-1][2], data_b, what)
        else:
            _same_bits(data_b, data, what + " against single pushes")
    return trace


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_script_through_both_entry_points(gpu_pkg, name):
    s = SCRIPTS[name]
    trace = _hold(gpu_pkg, s)
    assert trace[-1]["stats"]["ended"] > 0 and trace[-1]["stats"]["kept"] > 0


def test_the_largest_capacity_with_more_candidates_than_it_in_one_push(gpu_pkg):
    s = cases.large_k(LARGE_K, LARGE_N, "large_k", chunks=(3,))
    trace = _hold(gpu_pkg, s)
    assert trace[1]["stats"] == dict(kept=LARGE_K, ended=LARGE_N, admitted=LARGE_K, too_long=0)
    evicted = trace[3]["stats"]["admitted"] - LARGE_K
    assert 0.3 * LARGE_K < evicted < 0.7 * LARGE_K


def test_the_lanes_top_byte_decides_between_two_lanes_2_to_the_24_apart(gpu_pkg):
    """cases.LANE_TOP_BYTE: lanes 2^24 - 1 and 2^24 end in one push with one return and K = 1, so digit 12 of the key decides.  16.8 M
    lanes: nothing is copied to the host per step; the expected memory is written out by hand (history 1: the row is o_0 of the lane)."""
    import torch
    c = cases.LANE_TOP_BYTE
    n, steps, (low, high) = c["n"], c["steps"], c["lanes"]
    reward, done = np.zeros((steps, n), np.float32), np.zeros((steps, n), np.uint8)
    reward[steps - 1, [low, high]] = c["ret"]
    done[steps - 1, [low, high]] = 1
    stride = (n + 63) // 64 * 64
    for chunk in (0, 3):
        with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True) as env:
            env.ResetDevice()
            env.Tick = cases.TICK0
            mem = env.EpisodeMemory(capacity=c["capacity"], max_length=c["max_length"], history=1, rollout_chunk=chunk)
            rows = torch.empty((n, env.ObsDim), dtype=torch.float32, device="cuda")
            env.PackObsDevice(rows)
            env.Sync()
            first = rows[high].cpu().numpy()
            acts = torch.zeros((steps, stride), dtype=torch.int32, device="cuda")
            d_done = _dev(done)
            if chunk:
                obs = torch.empty((steps, env.ObsDim, n), dtype=torch.float32, device="cuda")
                rew = torch.empty((steps, n), dtype=torch.float32, device="cuda")
                rec_done = torch.empty((steps, n), dtype=torch.uint8, device="cuda")
                env.RolloutFusedDevice(acts, steps, stride, steps, rec_obs=obs, rec_reward=rew, rec_done=rec_done)
                env.Sync()
                rew.copy_(torch.from_numpy(reward))
                rec_done.copy_(d_done)
                torch.cuda.synchronize()
                mem.PushRollout(steps, obs, acts, rew, rec_done, action_stride=stride, ring=steps)
            else:
                for t in range(steps):
                    env.StepDevice(acts[t])
                    env.Sync()
                    env.SetArray("reward", reward[t])
                    mem.Push(acts[t], done=d_done[t])
            assert mem.Stats() == dict(kept=1, ended=2, admitted=1, too_long=0), chunk
            ret, length, tick, lane = mem.Episodes()
            assert (ret.tolist(), length.tolist(), tick.tolist(), lane.tolist()) == ([c["ret"]], [steps], [cases.TICK0 + steps], [high]), chunk
            x, action, onehot, r = (v.cpu().numpy() for v in mem.BuildDataset("params", min_episodes=0, reward=True))
            assert mem.DatasetSize() == 1 and np.array_equal(x[0].view(np.uint32), first.view(np.uint32)), chunk
            assert action.tolist() == [0] and onehot.tolist() == [[1.0, 0.0]] and r.tolist() == [0.0], chunk
