"""A NumPy restatement of the episode memory contract (include/gymnet_amd.h, gymnet_vecenv_memory_*): the reference's sequential
EndEpisode rule under the key order (return, end_tick, lane), the top-K-per-push form the device computes, and a whole memory fed with
what the step API returned (observations after the step, actions, rewards, done bytes) that yields the kept set and the dataset.

The model mirrors the device's bookkeeping: `obs[t]` is the observation stored for history index t (one index per push, plus the one
open at config), lane k's open episode started at index start[k], and a memory reset overwrites the pending index of the masked lanes.

The order of returns (include/gymnet_amd.h, "Keeping the best K"): +0 and -0 are one return; +-inf and denormals are ordinary values.  An
episode whose return is NaN is never kept, whatever the pool holds: it counts in `ended` and nowhere else (`too_long` goes by the length
alone).  Keys can be equal (a tick set backwards, a replay after Restore): the kept set is the top-K multiset of keys, every kept entry
is listed and built into the dataset exactly once, and among equal keys the order is the pool's — here the list's, an entry already kept
ahead of a newcomer."""
import numpy as np

# The scenario whose end ticks cross 2^32 (tests/test_gpu_episode_memory.py runs it on the device, tests/test_episode_memory_host.py drives
# the model through it with the NumPy oracle): the tick is set before the memory is configured, 40 pushes before the boundary.
TICKS_ACROSS_2_32 = dict(n=1024, capacity=100, max_steps=60, pushes=110, start_tick=2 ** 32 - 40)


def mixed_policy(n, rng, t, action_n=2):
    """The memory tests' Discrete actions: a fixed alternating policy, replaced by a uniform draw with probability 0.3."""
    a = rng.integers(0, action_n, n).astype(np.int32)
    greedy = (np.arange(n) + t) % action_n
    return np.where(rng.random(n) < 0.3, a, greedy).astype(np.int32)


def ticks_on_both_sides(m):
    """the pool holds end ticks below and at or above 2^32"""
    ticks = [e["tick"] for e in m.pool]
    return bool(ticks) and min(ticks) < 2 ** 32 <= max(ticks)


def ret_bits(ret):
    """A float32 return's place in the order, as an integer: +0 and -0 are one value, +-inf and denormals ordinary ones (the kernel's
    ret_bits, csrc/episode_memory_key.hpp).  A NaN has no place in it: no kept episode has one."""
    r = np.float32(ret)
    assert not np.isnan(r), "a NaN return is never kept, so it is never ordered"
    u = int(np.float32(0.0 if r == 0 else r).view(np.uint32))
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def is_nan(ret):
    return bool(np.isnan(np.float32(ret)))


def key(e):
    """The total order of kept episodes: (return, end_tick, lane); a later tick, then a higher lane, is newer and wins ties.  The
    return enters as its order bits, so the order is defined on every return a kept episode can have.  Equal keys can exist (a tick set
    backwards, a replay after Restore): the kept set is then the top-K MULTISET of keys, and among equal keys the entry already kept
    stays ahead of a newcomer."""
    return (ret_bits(e["ret"]), int(e["tick"]), int(e["lane"]))


def end_episode_sequential(pool, episode, capacity):
    """ReplayMemory.EndEpisode (MemoryTypes/ReplayMemory.cs:53-67) for ONE episode: add it when fewer than `capacity` are kept or its
    return is >= the lowest kept, then drop the lowest (by key; of equal keys the newest arrival) while more than `capacity` are kept.
    An episode whose return is NaN is never kept: the rule does not depend on what the pool holds."""
    if is_nan(episode["ret"]):
        return pool
    if len(pool) < capacity or float(episode["ret"]) >= min(float(e["ret"]) for e in pool):
        pool = pool + [episode]
    while len(pool) > capacity:
        low = min(range(len(pool)), key=lambda i: (key(pool[i]), -i))
        pool = pool[:low] + pool[low + 1:]
    return pool


def top_k_per_push(pool, ended, capacity):
    """What the device keeps after a push: the top `capacity` keys of (kept set + episodes that ended in that push with a return that
    is a number).  The sort is stable, so of equal keys the kept entries come first, in the pool's order."""
    return sorted(pool + [e for e in ended if not is_nan(e["ret"])], key=key, reverse=True)[:capacity]


class EpisodeMemoryModel:
    def __init__(self, obs0, capacity, max_length, history, autoreset=True):
        """obs0: [N, D] observations at config; every lane opens an episode from its own."""
        obs0 = np.asarray(obs0)
        self.n, self.d = obs0.shape
        self.capacity, self.max_length, self.history, self.autoreset = int(capacity), int(max_length), int(history), bool(autoreset)
        self.obs, self.act, self.rew = [obs0.copy()], [], []
        self.start = np.zeros(self.n, np.int64)
        self.length = np.zeros(self.n, np.int64)
        self.ret = np.zeros(self.n, np.float32)
        self.open = np.ones(self.n, bool)
        self.pool = []
        self.ended = self.admitted = self.too_long = 0

    def reset(self, obs, mask=None, clear=False):
        """memory_reset_device: masked lanes (all for None) open a new episode from `obs` at the pending history index."""
        sel = np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0
        self.obs[-1] = self.obs[-1].copy()
        self.obs[-1][sel] = np.asarray(obs)[sel]
        t = len(self.obs) - 1
        self.start[sel], self.length[sel], self.ret[sel], self.open[sel] = t, 0, np.float32(0), True
        if clear:
            self.pool = []
            self.ended = self.admitted = self.too_long = 0

    def push(self, actions, rewards, done, obs_after, end_tick):
        """One push after one vector step: actions [N], float32 rewards [N], done bytes [N], observations after the step [N, D] and the
        engine tick after the step.  Returns the episodes that ended in it."""
        t = len(self.obs) - 1
        self.act.append(np.asarray(actions).copy())
        self.rew.append(np.asarray(rewards, np.float32).copy())
        nxt = np.asarray(obs_after).copy()
        done = np.asarray(done) != 0
        live = self.open.copy()
        with np.errstate(invalid="ignore", over="ignore"):                 # inf - inf and overflow are returns like any other
            self.ret[live] = (self.ret[live] + self.rew[-1][live]).astype(np.float32)
        self.length[live] += 1
        ended = []
        for k in np.flatnonzero(live & done):
            self.ended += 1
            if self.length[k] > self.max_length:
                self.too_long += 1
                continue
            ended.append({"ret": np.float32(self.ret[k]), "len": int(self.length[k]), "tick": int(end_tick), "lane": int(k),
                          "start": int(self.start[k])})
        fin = live & done
        if self.autoreset:
            self.start[fin], self.length[fin], self.ret[fin] = t + 1, 0, np.float32(0)
        else:
            self.open[fin] = False
        self.obs.append(nxt)
        before = {id(e) for e in self.pool}
        self.pool = top_k_per_push(self.pool, ended, self.capacity)
        self.admitted += sum(1 for e in self.pool if id(e) not in before)
        return ended

    def kept(self):
        """The kept set in descending key order: (return float32, length, end_tick, lane) arrays."""
        p = sorted(self.pool, key=key, reverse=True)
        return (np.array([e["ret"] for e in p], np.float32), np.array([e["len"] for e in p], np.int32),
                np.array([e["tick"] for e in p], np.uint64), np.array([e["lane"] for e in p], np.int32))

    def steps(self, e):
        """The stored steps of a kept episode: obs [len, D], actions [len], rewards [len]."""
        idx = e["start"] + np.arange(e["len"])
        return (np.stack([self.obs[i][e["lane"]] for i in idx]), np.array([self.act[i][e["lane"]] for i in idx]),
                np.array([self.rew[i][e["lane"]] for i in idx], np.float32))

    def dataset_rows(self):
        """(episode, step p, history indices of o_{p-S+1} .. o_p clamped to o_0) of every dataset row, in order (DataBuilder.cs:25-55)."""
        rows = []
        for e in sorted(self.pool, key=key, reverse=True):
            for p in range(e["len"] * 2 // 3):
                hist = [e["start"] + max(p - (self.history - 1) + s, 0) for s in range(self.history)]
                rows.append((e, p, hist))
        return rows

    def dataset_params(self, action_n=None):
        """x float32 [rows, S * D], actions [rows], one-hot float32 [rows, action_n] (None for Box), rewards float32 [rows]."""
        rows = self.dataset_rows()
        x = np.zeros((len(rows), self.history * self.d), np.float32)
        a = np.zeros(len(rows), self.act[0].dtype if self.act else np.int32)
        r = np.zeros(len(rows), np.float32)
        for i, (e, p, hist) in enumerate(rows):
            x[i] = np.concatenate([self.obs[h][e["lane"]] for h in hist]).astype(np.float32)
            a[i] = self.act[e["start"] + p][e["lane"]]
            r[i] = self.rew[e["start"] + p][e["lane"]]
        onehot = None
        if action_n:
            onehot = np.zeros((len(rows), action_n), np.float32)
            onehot[np.arange(len(rows)), a.astype(np.int64)] = 1.0
        return x, a, onehot, r
