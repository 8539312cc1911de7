"""Adversarial scripts for the episode memory's key order (tests/test_episode_memory_keys_host.py states what they cover,
tests/test_gpu_episode_memory_keys.py runs them on the device).  Pure: fixed seeds and hand-written tables, no device, no files.

A script is a memory configuration (n lanes, capacity K, max_length L, history, env, dtype) and a list of segments.  A segment is T
vector steps whose per-step reward rows [T][N] (float32 BIT PATTERNS, uint32) and done rows [T][N] (uint8) the test puts in place of
the env's own; the observations and actions are whatever the env produces — payload.  The memory computes each return as the float32
sum of the lane's rewards in step order, so a script chooses its returns: one step carries the value, the others +0 (0 + v == v
exactly; -0 as a reward gives the return +0, for 0.0f + -0.0f is +0: no sum of rewards is -0), +inf followed by -inf gives NaN.
Every segment starts at an explicit engine tick: the first before the memory is configured, a later one after `restore` (the handle goes
back to the checkpoint taken at the start of the segment flagged `checkpoint`) or after the tick was set, forwards or backwards; every
later segment opens every lane again (memory reset).  Step t of a segment ends its episodes at tick + t + 1.

model_trace() drives tests/_episode_memory_model.py through a script and returns what every push saw, for the coverage conditions and
for the device comparison."""
import numpy as np

import _episode_memory_model as model

NEG = 0x80000000
POS0, NEG0, DEN, FMIN, ONE, FMAX, INF = 0x00000000, 0x80000000, 0x00000001, 0x00800000, 0x3F800000, 0x7F7FFFFF, 0x7F800000
NANS = {"+qnan": (0x7FC00000,), "-qnan": (0xFFC00000,), "+payload": (0x7FC00001,), "-payload": (0xFFC12345,), "inf-inf": (INF, NEG | INF)}
# every return at the sign fold, ascending (the reward -0 gives the return +0: it ties with +0 and the tick or lane decides)
FOLD = [NEG | INF, NEG | FMAX, NEG | (ONE + 1), NEG | ONE, NEG | (ONE - 1), NEG | FMIN, NEG | DEN, NEG0, POS0, DEN, FMIN, ONE - 1, ONE, ONE + 1,
        FMAX, INF]
TIE_LANES = [0, 1, 255, 256, 65535, 65536]
TICK0 = 0x1000
# two lanes 2^24 apart end in one push with one return: the only way the lane's top byte (digit 12) decides a selection.  Too large for
# the generic runner's per-step host copies: the GPU test has a case of its own for it.
LANE_TOP_BYTE = dict(n=(1 << 24) + 1, lanes=((1 << 24) - 1, 1 << 24), capacity=1, max_length=2, steps=2, ret=7.0)
FAMILIES = ("sign_fold", "one_digit", "ties", "nan", "capacity", "large_k", "stale", "equal_keys")


def bits(x):
    return int(np.float32(x).view(np.uint32))


def as_float(b):
    return np.uint32(b).view(np.float32)


def order_word_to_bits(w):
    """the float32 bit pattern whose order word (ret_bits) is w, or None when no return has it (a NaN, or -0)"""
    b = (w ^ NEG) if w & NEG else (~w & 0xFFFFFFFF)
    f = as_float(b)
    return None if np.isnan(f) or b == NEG0 else b


def value_at(value, length, at):
    """the rewards of an episode of `length` steps whose return is the value(s): +0 everywhere but from step `at` on"""
    value = tuple(value) if isinstance(value, (tuple, list)) else (value,)
    at = min(at, length - len(value))
    assert at >= 0
    return [POS0] * at + list(value) + [POS0] * (length - at - len(value))


def marked(marker, ret, length):
    """rewards with a marker in step 0 that still sum to `ret` (small integers: every partial sum is exact)"""
    assert length >= 2
    return [bits(marker)] + [POS0] * (length - 2) + [bits(ret - marker)]


class Rows:
    """the reward and done rows of one segment, written episode by episode"""

    def __init__(self, n, steps):
        self.reward = np.zeros((steps, n), np.uint32)
        self.done = np.zeros((steps, n), np.uint8)
        self.last = {}

    def episode(self, lane, t_end, rewards):
        """an episode of len(rewards) steps on `lane` that ends in step t_end: it begins where the lane's previous one ended"""
        first = t_end - len(rewards) + 1
        assert first == self.last.get(lane, -1) + 1, (lane, t_end, len(rewards))
        self.reward[first:t_end + 1, lane] = rewards
        self.done[t_end, lane] = 1
        self.last[lane] = t_end

    def ends(self, lane, t_end, value, at=None):
        """the lane's next episode ends in step t_end with the return `value` (bit pattern, or several: consecutive rewards)"""
        length = t_end - self.last.get(lane, -1)
        self.episode(lane, t_end, value_at(value, length, length - 1 if at is None else at))


def segment(rows, tick, **kw):
    seg = dict(tick=int(tick), reward=rows.reward, done=rows.done, restore=False, checkpoint=False, action_seed=None)
    seg.update(kw)
    return seg


def script(name, family, n, capacity, max_length, segments, **kw):
    s = dict(name=name, family=family, n=n, capacity=capacity, max_length=max_length, history=2, env="CartPole-v1", dtype="float32",
             chunks=(1, 3, 16), equal_keys=None, markers=None, sequential=True)
    s.update(kw)
    s["segments"] = segments
    for i, seg in enumerate(segments):
        if seg["action_seed"] is None:
            seg["action_seed"] = i
    return s


# ---- the families --------------------------------------------------------------------------------------------------------------------
def sign_fold():
    out = []
    # every fold value in one pool, then fifteen pushes that each evict the lowest: the K-th key sits between every neighbouring pair
    n = 257
    r = Rows(n, 18)
    for i, v in enumerate(FOLD):
        r.ends(i * 37 % n, 2, v, at=i % 3)
    for j in range(15):
        r.ends(200 + j, 3 + j, INF, at=j % 3)
    out.append(script("fold_all", "sign_fold", n, 16, 24, [segment(r, TICK0)]))
    # K = 1, ascending: every return is admitted over its lower neighbour by the push's filter (the two zeros tie: the newer wins)
    r = Rows(64, 16)
    for t, v in enumerate(FOLD):
        r.ends(t, t, v, at=t // 2)
    out.append(script("fold_up", "sign_fold", 64, 1, 16, [segment(r, TICK0)]))
    # K = 2, descending: after the first two, every return is refused by the filter against its upper neighbour
    r = Rows(64, 16)
    for t, v in enumerate(reversed(FOLD)):
        r.ends(63 - t, t, v, at=0)
    out.append(script("fold_down", "sign_fold", 64, 2, 16, [segment(r, TICK0)]))
    # all sixteen in one push, K on either side of the pair of zeros and between them; then again in a later push
    for k in (7, 8, 9):
        n = 1027
        r = Rows(n, 4)
        for i, v in enumerate(FOLD):
            r.ends(i * 211 % n, 1, v, at=i % 2)
            r.ends((i * 211 + 5) % n, 3, v, at=i % 4)
        out.append(script(f"fold_k{k}", "sign_fold", n, k, 4, [segment(r, TICK0)]))
    return out


def one_digit():
    """returns whose order words differ from a base in one byte only, and carries ..FF against ..00 below each byte"""
    out = []
    base = 0xBF4A3C2D
    for j in range(4):
        sh = 24 - 8 * j
        words = {base}
        for v in (0x00, 0x01, 0x7F, 0x80, 0xFE, 0xFF):
            words.add((base & ~(0xFF << sh) & 0xFFFFFFFF) | (v << sh))
        low = (1 << (sh + 8)) - 1                       # this byte and everything below it
        carry = base | low
        words.update({carry, (carry + 1) & 0xFFFFFFFF})
        vals = sorted(b for b in (order_word_to_bits(w) for w in words) if b is not None)
        rng = np.random.default_rng(100 + j)
        vals = [vals[i] for i in rng.permutation(len(vals))]
        r = Rows(64, 2 + len(vals) - 5)
        for i, v in enumerate(vals[:5]):
            r.ends(3 + 7 * i, 1, v, at=i % 2)
        for i, v in enumerate(vals[5:]):
            r.ends(40 + i, 2 + i, v, at=i)
        out.append(script(f"one_digit_byte{j}", "one_digit", 64, 3, 16, [segment(r, TICK0)]))
    return out


def ties():
    """all returns equal: the tick, then the lane decides.  Six lanes end in one push; the segments' start ticks differ in one byte
    after another, so the end ticks of two segments differ only there."""
    out = []
    n = TIE_LANES[-1] + 65                              # 65601: a last workgroup of 65 lanes
    seven = bits(7.0)

    def rows():
        r = Rows(n, 2)
        for lane in TIE_LANES:
            r.ends(lane, 1, seven, at=0)
        return r
    ticks = [TICK0] + [TICK0 + (1 << s) for s in (8, 16, 24, 32, 40, 48, 56, 63)]
    # K = 6: each segment's six episodes replace the previous segment's, ret == thr in a full pool, decided by a tick byte
    out.append(script("ties_tick", "ties", n, 6, 2, [segment(rows(), t) for t in ticks], chunks=(3,)))
    for k in (1, 3, 5):                                 # the K-th key between lanes 65536|65535, 256|255, 1|0
        out.append(script(f"ties_lane_k{k}", "ties", n, k, 2, [segment(rows(), t) for t in ticks[:2]], chunks=(1, 16)))
    return out


def nan_scripts():
    """NaN returns while the pool is empty, half full and full, alone in a push and beside ordinary episodes; ordinary episodes after them"""
    kinds = list(NANS.values())

    def build(name, **kw):
        n = 257
        r = Rows(n, 12)
        for i, kind in enumerate(kinds):                # step 3, pool empty: every kind in the first, a middle and the last step
            for p, at in enumerate((0, 1, 3)):
                r.ends(3 * i + p, 3, kind, at=at)
        r.ends(20, 4, NANS["-qnan"])                    # step 4: the only candidate of its push, pool still empty
        r.ends(30, 5, bits(1.0)); r.ends(31, 5, bits(2.0))                              # half full
        for i, kind in enumerate(kinds):                # step 6, half full: NaN beside an ordinary episode
            r.ends(i, 6, kind, at=i % 3)
        r.ends(32, 6, bits(3.0))
        r.ends(33, 7, bits(0.5))                        # full: 3, 2, 1, 0.5
        for i, kind in enumerate(kinds):                # step 8, full: NaN beside an ordinary episode that evicts
            r.ends(5 + i, 8, kind, at=i)
        r.ends(30, 8, bits(1.5))
        r.ends(10, 9, NANS["-qnan"], at=2); r.ends(11, 9, NANS["+qnan"], at=0)          # full: NaN alone in the push
        r.ends(31, 10, bits(5.0)); r.ends(12, 10, NANS["inf-inf"], at=3)                # ordinary episodes are still admitted
        r.ends(32, 11, bits(1.5))                       # ... also on ret == thr
        return script(name, "nan", n, 4, 8, [segment(r, TICK0)], **kw)
    return [build("nan_states"), build("nan_states_f64", dtype="float64", chunks=(3,)),
            build("nan_states_pendulum", env="Pendulum-v1", chunks=(16,))]


def capacity():
    out = []
    rng = np.random.default_rng(7)
    r = Rows(64, 4)                                     # K = 1
    r.ends(3, 0, bits(2.0)); r.ends(4, 1, bits(1.0)); r.ends(5, 1, bits(3.0)); r.ends(6, 2, bits(3.0)); r.ends(3, 3, bits(2.5))
    out.append(script("cap_k1", "capacity", 64, 1, 8, [segment(r, TICK0)]))
    n = 257                                             # total < K, == K, == K + 1, a refused one, more candidates than K
    r = Rows(n, 5)
    for lane, v in ((0, 5.0), (100, 3.0), (256, 8.0)):
        r.ends(lane, 0, bits(v))
    r.ends(1, 1, bits(4.0)); r.ends(255, 1, bits(6.0))
    r.ends(2, 2, bits(5.5))
    r.ends(3, 3, bits(3.5))
    for i in range(8):
        r.ends(10 + 30 * i, 4, bits(float(2 + i)))
    out.append(script("cap_total", "capacity", n, 5, 8, [segment(r, TICK0)]))
    r = Rows(n, 4)                                      # every lane a candidate of one push, twice
    for t in (1, 3):
        vals = rng.permutation(n * 4)[:n] - n
        for lane in range(n):
            r.ends(lane, t, bits(float(vals[lane]) * 0.25), at=lane % 2)
    out.append(script("cap_burst", "capacity", n, 4, 4, [segment(r, TICK0)]))
    r = Rows(64, 5)                                     # L = 1: every lane ends in every push, no episode has a dataset row
    for t in range(5):
        for lane in range(64):
            r.ends(lane, t, bits(float(rng.integers(0, 6))))
    out.append(script("cap_l1", "capacity", 64, 10, 1, [segment(r, TICK0)]))
    r = Rows(64, 6)                                     # L = 2: episodes of no row (1 step) and of one row (2 steps) side by side
    for t in range(6):
        for lane in range(64):
            if lane % 2 == 0 or t % 2 == 1:
                r.ends(lane, t, bits(float(rng.integers(0, 6))), at=0)
    out.append(script("cap_l2", "capacity", 64, 10, 2, [segment(r, TICK0)]))
    r = Rows(64, 6)                                     # len == L is kept, len == L + 1 is too long whatever it returns
    r.ends(1, 3, bits(1.0)); r.ends(2, 4, bits(100.0)); r.ends(3, 4, bits(-1.0), at=0); r.ends(1, 5, bits(0.5)); r.ends(4, 5, INF)
    out.append(script("cap_len", "capacity", 64, 4, 4, [segment(r, TICK0)]))
    return out


def large_k(k, n, name, **kw):
    """every lane ends in one push (more than K candidates for an empty pool), then again: about half of the pool is evicted"""
    rng = np.random.default_rng(k + n)
    r = Rows(n, 4)
    for t in (1, 3):
        vals = rng.standard_normal(n).astype(np.float32).view(np.uint32)
        r.reward[t, :] = vals
        r.done[t, :] = 1
    return script(name, "large_k", n, k, 4, [segment(r, TICK0)], **kw)


def stale():
    """a pool below K before an ingest pass (of 3 or of 16 steps) that fills in step 3; the later steps of the pass hold a candidate
    below the new lowest return, one equal to it, a NaN, and steps whose candidates all fall below it"""
    def build(name, nan, **kw):
        n = 257
        r = Rows(n, 20)
        r.ends(0, 0, bits(10.0)); r.ends(1, 0, bits(20.0))
        r.ends(2, 3, bits(30.0)); r.ends(3, 3, bits(40.0), at=1); r.ends(4, 3, bits(5.0))
        r.ends(5, 4, bits(7.0)); r.ends(6, 4, bits(10.0), at=0); r.ends(7, 4, NANS[nan], at=2)
        r.ends(8, 5, bits(1.0)); r.ends(256, 5, bits(2.0))
        r.ends(10, 6, bits(9.0))
        r.ends(11, 9, bits(50.0))
        r.ends(12, 17, bits(20.0)); r.ends(13, 17, bits(15.0))
        r.ends(0, 19, bits(60.0))
        return script(name, "stale", n, 4, 24, [segment(r, TICK0)], **kw)
    # (a positive NaN would rank above +inf if it got as far as the selection, a negative one below -inf)
    return [build("stale", "+qnan", chunks=(3, 16)), build("stale_f64", "-qnan", dtype="float64", chunks=(3, 16)),
            build("stale_pendulum", "+payload", env="Pendulum-v1", chunks=(3, 16))]


def equal_keys():
    """the same (return, tick, lane) twice: a replay after Restore (identical rows), and a tick set backwards (other rows, told apart by
    the marker in step 0).  K = 5 over the keys a a b b c c d d keeps a a b b c: the K-th key has an equal below it."""
    out = []
    n = 257
    for kind in ("replay", "backwards"):
        markers = {}

        def first(offset):
            r = Rows(n, 6)
            for i, (lane, t, ret) in enumerate(((10, 2, 4.0), (20, 3, 3.0), (30, 4, 2.0), (256, 5, 1.0))):
                r.episode(lane, t, marked(offset + i + 1, ret, t + 1))
                markers[offset + i + 1] = (ret, TICK0 + t + 1, lane, t + 1)
            return r
        r2 = Rows(n, 3)
        r2.episode(70, 1, marked(70, 2.0, 2)); markers[70] = (2.0, TICK0 + 6 + 2, 70, 2)       # ret == thr: the newer one replaces c
        r2.episode(50, 2, marked(50, 3.5, 3)); markers[50] = (3.5, TICK0 + 6 + 3, 50, 3)
        r2.episode(60, 2, marked(60, 3.0, 3)); markers[60] = (3.0, TICK0 + 6 + 3, 60, 3)
        segs = [segment(first(0), TICK0, checkpoint=True, action_seed=0),
                segment(first(0 if kind == "replay" else 100), TICK0, restore=kind == "replay", action_seed=0 if kind == "replay" else 1),
                segment(r2, TICK0 + 6, action_seed=2)]
        out.append(script(f"equal_{kind}", "equal_keys", n, 5, 8, segs, equal_keys=kind, markers=markers))
    return out


def scripts():
    """every script but the full-size large-K ones (large_k() builds those for the GPU test)"""
    return (sign_fold() + one_digit() + ties() + nan_scripts() + capacity() + [large_k(512, 600, "large_k_small")] + stale() + equal_keys())


# ---- the model, driven through a script ----------------------------------------------------------------------------------------------
def key_digits(e):
    """the 16 digits of an episode's key, most significant first"""
    rb, tick, lane = model.key(e)
    return list(rb.to_bytes(4, "big") + tick.to_bytes(8, "big") + lane.to_bytes(4, "big"))


def deciding_digit(before, ended, capacity):
    """the first digit in which the K-th and the (K + 1)-th largest key of a push differ: the one its selection turns on (None: no
    selection, or the two keys are equal)"""
    every = sorted(before + [e for e in ended if not model.is_nan(e["ret"])], key=model.key, reverse=True)
    if len(every) <= capacity:
        return None
    a, b = key_digits(every[capacity - 1]), key_digits(every[capacity])
    return next((d for d in range(16) if a[d] != b[d]), None)


def model_trace(s, feed=None):
    """Runs the model through script s.  feed[i] = (obs0 [N, D], actions [T][N], obs_after [T][N, D]) of segment i as the device
    produced them (None: zeros — the kept set does not depend on them).  Returns the model and one record per push: segment, step, the
    pool before, the episodes that ended (not too long; NaN ones included), the pool and the counters after."""
    n, m, trace = s["n"], None, []
    for i, seg in enumerate(s["segments"]):
        steps = seg["reward"].shape[0]
        if feed is None:
            obs0, acts, after = np.zeros((n, 1), np.float32), np.zeros((steps, n), np.int32), [np.zeros((n, 1), np.float32)] * steps
        else:
            obs0, acts, after = feed[i]
        if m is None:
            m = model.EpisodeMemoryModel(obs0, s["capacity"], s["max_length"], s["history"])
        else:
            m.reset(obs0)
        for t in range(steps):
            before = list(m.pool)
            ended = m.push(acts[t], seg["reward"][t].view(np.float32), seg["done"][t], after[t], seg["tick"] + t + 1)
            trace.append(dict(segment=i, step=t, before=before, ended=ended, pool=list(m.pool),
                              stats=dict(kept=len(m.pool), ended=m.ended, admitted=m.admitted, too_long=m.too_long)))
    return m, trace
