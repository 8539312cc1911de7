"""GPU checks of the fused actor rollout's forms and edges (gym.net_amd/csrc/actor.hip).  Every comparison is bit for bit (logits: -0 == +0).

What is compared with what:
  * each of the 18 actor_rollout_kernel<Env,AUTORESET,EXTRAS,RECORDS> forms of tests/_actor_forms.py FORMS, reached through the public API,
    with a twin handle that runs T x (Act, StepDevice, Push) — the step kernels, which the oracle covers: recorded actions, observations,
    rewards and dones, state, done bytes, tick, history, episode statistics, episode records as sets, count[1]; without auto-reset also
    CartPole's steps_beyond_done, the stepped-after-done counter and the rewards of the lanes that step after done;
  * the record staging against the same twin: more than kStageRecords (256) records per wave so that the stage is flushed inside the
    loop, partial waves down to one active lane, a capacity equal to the truth, and the overflow spill of a shard whose segment is full
    with capacity equal to the truth and one below it;
  * Act's logits and greedy actions with the fmaf twin (tests/_actor_twin.py) at the deepest histories, the widest and the narrowest
    layers, four layers and exactly tied logits; the fused rollout with the twin handle at depth 1, the deepest depth of each env, T < S
    and T % S != 0, starting from a ring slot other than 0;
  * a handle tick and an action tick that cross 2^32 and an action seed above 2^32: fused against single steps, and the single steps
    against a replay with the oracle's step, reset draw and action-stream words;
  * lane offsets: one handle of 2048 lanes against two handles of 1000 and 1048 lanes at offsets 0 and 1000."""
import numpy as np
import pytest

import _actor_forms as forms
import _actor_twin as twin

pytestmark = pytest.mark.gpu
SEED = 0xAC7
DIMS = {"CartPole-v1": (4, 2), "MountainCar-v0": (2, 3), "Acrobot-v1": (6, 3)}           # env -> (obs_dim, actions)


def _widths(name, S):
    O, A = DIMS[name]
    return [S * O] + forms.HIDDEN[name] + [A]


# ---- 1. every form ---------------------------------------------------------------------------------------------------------------------

def _at_the_goal(env):
    """MountainCar / Acrobot lanes do not end within 40 steps on their own: every third lane starts where its next step is terminal
    (MountainCar: 0.49 with velocity 0.05; Acrobot: both links straight up), so a handle without auto-reset steps them after done."""
    s = env.GetState()
    third = np.arange(s.shape[1]) % 3 == 0
    if env.StateDim == 2:
        s[0, third], s[1, third] = 0.49, 0.05
    else:
        s[:, third] = np.array([np.pi, 0.0, 0.0, 0.0], np.float32)[:, None]
    env.SetState(s)


@pytest.mark.parametrize("row", forms.FORMS, ids=forms.form_id)
def test_every_rollout_form_equals_single_steps(gpu_pkg, row, n=1000, T=40):
    name = row["env"]
    rng = np.random.default_rng(len(row["kernel"]) + T)
    w, flat, pairs = twin.net(rng, _widths(name, 4))
    prepare = _at_the_goal if (not row["auto_reset"] and name != "CartPole-v1") else None
    out = forms.fused_equals_single_steps(gpu_pkg, name, n, T, forms.handle_kwargs(row), row["shape"] == "records", pairs, S=4, eps=0.3,
                                          prepare=prepare, env_seed=SEED)
    if row["shape"] == "records":
        assert out["ended"] > 0
    if not row["auto_reset"]:
        done = out["done"] != 0
        before = np.logical_or.accumulate(done, axis=0)[:-1]                  # [t]: done at or before step t, t < T - 1
        assert before[-1].mean() >= 0.25                                      # a quarter of the lanes were done before the last step
        after = np.zeros_like(done)
        after[1:] = before                                                    # the steps a lane takes after it was done
        assert after.sum() >= 0.25 * n
        if name == "CartPole-v1":                     # CartPoleEnv.cs:176-183: reward 0 for a terminal step after a terminal step, and counted
            term = (out["done"] & 1) != 0                                     # (bit 1 is the time limit's, which the env does not see)
            again = np.zeros_like(term)
            again[1:] = np.logical_or.accumulate(term, axis=0)[:-1]
            assert (out["reward"][again & term] == 0.0).all() and (again & term).sum() >= 0.25 * n
            assert out["stepped_after_done"] > 0 and (out["steps_beyond_done"] > 0).mean() >= 0.25


# ---- 2. record staging -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [640, 1, 63, 65])
def test_record_stage_flushes_inside_the_loop(gpu_pkg, n, T=64):
    """max_episode_steps = 3: every lane ends at least 21 episodes in 64 steps, so a full wave stages >= 1344 records and flushes its 256-record
    stage five times or more inside the loop; n = 1, 63, 65: partial waves, with one active lane draining the whole stage at n = 1."""
    rng = np.random.default_rng(n)
    w, flat, pairs = twin.net(rng, _widths("CartPole-v1", 4))
    kw = dict(auto_reset=True, episode_stats=True, max_episode_steps=3)
    out = forms.fused_equals_single_steps(gpu_pkg, "CartPole-v1", n, T, kw, True, pairs, capacity="exact", env_seed=SEED)
    per_lane = (out["done"] != 0).sum(axis=0)
    assert per_lane.min() >= 21
    assert out["kept"] == out["ended"] == len(out["want"]) == per_lane.sum()


def test_records_spill_to_the_overflow_segment_with_the_actor_choosing(gpu_pkg):
    """tests/test_gpu_fused_rollout_ex.py's skewed-lanes case with the actor choosing the actions: 300 waves, and only waves 0 and 256 — the
    same shard — start with theta = 0.2, theta_dot = 1.0 and end at the first step under either action; an upright lane cannot end before step
    index 8 and a freshly reset one not before 7, so six steps end exactly 128 episodes, all in shard 0, whose segment holds 66."""
    n, T = 64 * 300, 6
    rng = np.random.default_rng(6)
    w, flat, pairs = twin.net(rng, _widths("CartPole-v1", 4))
    s = np.zeros((4, n), np.float32)
    hot = np.r_[0:64, 64 * 256:64 * 257]
    s[2, hot], s[3, hot] = 0.2, 1.0
    kw = dict(auto_reset=True, episode_stats=True)

    def run(capacity):
        return forms.fused_equals_single_steps(gpu_pkg, "CartPole-v1", n, T, kw, True, pairs, prepare=lambda env: env.SetState(s),
                                               capacity=capacity, env_seed=SEED)
    roomy = run(1 << 16)
    truth = roomy["ended"]
    per_shard = 2 * ((truth + 255) // 256) + 64
    assert truth == 128 and truth > per_shard
    assert roomy["kept"] == truth and {r[1] for r in roomy["got"]} == set(hot.tolist()) and {r[0] for r in roomy["got"]} == {0}
    exact = run(truth)
    assert (exact["kept"], exact["ended"]) == (128, 128) and exact["got"] == roomy["got"]
    short = run(truth - 1)
    assert (short["kept"], short["ended"]) == (127, 128) and set(short["got"]) <= set(roomy["got"]) and len(set(short["got"])) == 127


# ---- 3. history depth and network shape edges ----------------------------------------------------------------------------------------

def _act_against_the_twin(gpu_pkg, name, S, w, flat, n=777, warm=5):
    """(logits, actions) of Act after `warm` random steps with pushes, asserted equal to the fmaf twin over the handle's own history"""
    import torch
    rng = np.random.default_rng(S + n)
    with gpu_pkg.VectorEnv(name, n, seed=SEED, auto_reset=True) as env:
        env.Reset()
        A = env.ActionSpace.N
        actor = env.Actor(twin.layers(w, flat), history=S)
        for t in range(warm):
            acts = torch.from_numpy(rng.integers(0, A, n).astype(np.int32)).cuda()
            torch.cuda.synchronize()                                          # the handle steps on a stream of its own
            env.StepDevice(acts)
            actor.Push()
        logits = torch.empty((n, A), dtype=torch.float32, device="cuda")
        act = forms.host(actor.Act(logits=logits))
        x = actor.History().reshape(n, -1)
        want_l, want_g = twin.forward(w, flat, x)
        got_l = forms.host(logits)
        assert twin.same(got_l, want_l)
        assert np.array_equal(act, want_g)
        return got_l, act, x


SHAPE_EDGES = [("CartPole-v1", 16, [64, 64, 57, 2]),           # 7981 parameters (the cap is 8192); width 64 in and out: every chunk and group live
               ("CartPole-v1", 4, [16, 64, 33, 1, 2]),         # four layers; a hidden width of 1
               ("CartPole-v1", 1, [4, 5, 9, 2]),               # widths 4k + 1 and 8k + 1
               ("Acrobot-v1", 10, [60, 7, 3]),                 # 60 inputs: the four-input tail of x stays zero
               ("MountainCar-v0", 32, [64, 4, 8, 3])]          # exact multiples of 4 and 8


@pytest.mark.parametrize("name,S,widths", SHAPE_EDGES, ids=[f"{e[0]}-{e[1]}-" + "x".join(map(str, e[2])) for e in SHAPE_EDGES])
def test_act_at_the_shape_edges_equals_the_twin(gpu_pkg, name, S, widths):
    w, flat = twin.random_net(np.random.default_rng(sum(widths)), widths, scale=2.0)
    assert flat.size <= 8192
    for W, b in twin.layers(w, flat):
        if len(b) == 1:
            b[0] = 1.0                                                        # (a view into flat) keep the single hidden unit alive
    logits, act, x = _act_against_the_twin(gpu_pkg, name, S, w, flat, warm=S + 3)
    O = DIMS[name][0]
    assert len(np.unique(logits[:, 0])) > 1 and (S == 1 or (x[:, :O] != x[:, -O:]).any())      # the lanes differ, and so do the slots


DEPTH_EDGES = [("CartPole-v1", 1, 5, 3),                       # depth 1
               ("CartPole-v1", 16, 7, 5),                      # T < S: the ring is not fully rotated
               ("CartPole-v1", 16, 37, 29),                    # wraps twice, T % S != 0
               ("Acrobot-v1", 10, 23, 17),                     # the deepest depth for 6 observations
               ("MountainCar-v0", 32, 40, 29)]                 # the deepest depth for 2 observations


@pytest.mark.parametrize("name,S,T,limit", DEPTH_EDGES)
def test_fused_rollout_at_the_depth_edges_equals_single_steps(gpu_pkg, name, S, T, limit, n=777):
    """the time limit (below T) ends episodes in every env, so both the append and the refill of the ring run; three warm-up steps start the
    rollout at ring slot 3 % S"""
    w, flat, pairs = twin.net(np.random.default_rng(S * T), _widths(name, S))
    kw = dict(auto_reset=True, episode_stats=True, max_episode_steps=limit)
    out = forms.fused_equals_single_steps(gpu_pkg, name, n, T, kw, True, pairs, S=S, warm=3, env_seed=SEED)
    assert out["ended"] >= n and (out["done"] == 0).any()


def test_two_equal_output_rows_choose_action_0(gpu_pkg):
    rng = np.random.default_rng(21)
    w, flat = twin.random_net(rng, [16, 8, 2], scale=2.0)
    pairs = twin.layers(w, flat)
    pairs[1][0][1], pairs[1][1][1] = pairs[1][0][0], pairs[1][1][0]            # (views into flat) row 1 = row 0, bias included
    logits, act, _ = _act_against_the_twin(gpu_pkg, "CartPole-v1", 4, w, flat)
    assert np.array_equal(logits[:, 0].view(np.uint32), logits[:, 1].view(np.uint32)) and (logits[:, 0] != 0).any()
    assert (act == 0).all()


def test_a_duplicated_maximum_chooses_its_first_index(gpu_pkg):
    rng = np.random.default_rng(22)
    w, flat = twin.random_net(rng, [24, 8, 3], scale=2.0)
    pairs = twin.layers(w, flat)
    pairs[1][0][2], pairs[1][1][2] = pairs[1][0][1], pairs[1][1][1]            # row 2 = row 1
    pairs[1][0][0], pairs[1][1][0] = -pairs[1][0][1], -pairs[1][1][1]          # row 0 = their negation
    logits, act, _ = _act_against_the_twin(gpu_pkg, "Acrobot-v1", 4, w, flat)
    assert np.array_equal(logits[:, 1].view(np.uint32), logits[:, 2].view(np.uint32))
    assert np.array_equal(act, np.where(logits[:, 1] > 0, 1, 0)) and not (act == 2).any()
    assert (act == 0).any() and (act == 1).any()


# ---- 4. 64-bit counters and lane offsets ----------------------------------------------------------------------------------------------

def test_ticks_and_seed_across_2_to_the_32(gpu_pkg, oracle, n=256, T=7):
    """The handle's tick starts at 2^32 - 3 and the action tick at 2^32 - 2, the action seed is above 2^32, the time limit of 3 makes
    every lane reset at ticks 2^32 - 1 and 2^32 + 2: fused equals single steps, and the single steps equal the oracle's replay."""
    S, eps, aseed, tick0, start, limit = 4, 0.3, 0x1_0000_0063, 2 ** 32 - 2, 2 ** 32 - 3, 3
    w, flat, pairs = twin.net(np.random.default_rng(32), _widths("CartPole-v1", S))
    kw = dict(auto_reset=True, episode_stats=True, max_episode_steps=limit)

    def set_tick(env):
        env.Tick = start
    out = forms.fused_equals_single_steps(gpu_pkg, "CartPole-v1", n, T, kw, True, pairs, S=S, eps=eps, seed=aseed, tick0=tick0, prepare=set_tick,
                                          env_seed=SEED)
    s = oracle.cartpole_reset(SEED, 0, 0, n)                                  # Reset() ran at tick 0, before the tick was set
    model = twin.History(s.T, S)
    length = np.zeros(n, np.int64)
    resets = set()
    for t in range(T):
        tick = start + t
        _, greedy = twin.forward(w, flat, model.x())
        want_a = oracle.compose_discrete(aseed, 0, tick0 + t, 2, eps, greedy)
        wb = oracle.action_words(aseed, 0, tick0 + t, n)[1]                   # the high words matter: truncated, the coins differ
        assert not np.array_equal(wb, oracle.action_words(aseed & 0xFFFFFFFF, 0, tick0 + t, n)[1])
        if tick0 + t >= 2 ** 32:
            assert not np.array_equal(wb, oracle.action_words(aseed, 0, (tick0 + t) & 0xFFFFFFFF, n)[1])
        assert np.array_equal(out["actions"][t], want_a), t
        s, r, d, _ = oracle.cartpole_step(s, want_a, dtype=np.float32)
        length += 1
        done = d | np.where(length >= limit, 2, 0).astype(np.uint8)
        fin = done != 0
        s[:, fin] = oracle.cartpole_reset(SEED, 0, tick, n)[:, fin]
        length[fin] = 0
        if fin.any():
            resets.add(tick)
        assert np.array_equal(out["obs"][t].view(np.uint32), s.view(np.uint32)), t
        assert np.array_equal(out["reward"][t], r) and np.array_equal(out["done"][t], done), t
        model.push(s.T, done)
    assert min(resets) < 2 ** 32 <= max(resets)                               # reset draws on both sides of the boundary
    assert not np.array_equal(oracle.cartpole_reset(SEED, 0, 2 ** 32 + 2, n), oracle.cartpole_reset(SEED, 0, 2, n))


def test_lane_offset_splits_one_handle_into_two(gpu_pkg, T=20):
    """1000 is no multiple of 64: the second part's waves hold other lanes than the whole handle's, and compose_one's wave-level skip of the
    action word must not show."""
    import torch
    n1, n2 = 1000, 1048
    w, flat, pairs = twin.net(np.random.default_rng(40), _widths("CartPole-v1", 4))

    def run(n, lane_offset):
        with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True, lane_offset=lane_offset) as env:
            env.Reset()
            env.Actor(pairs, 4)
            rec = dict(rec_obs=torch.empty((T, 4, n), dtype=torch.float32, device="cuda"), rec_done=torch.empty((T, n), dtype=torch.uint8, device="cuda"),
                       rec_actions=torch.empty((T, n), dtype=torch.int32, device="cuda"))
            env.RolloutFusedDevice(None, T, actions="actor", epsilon=0.3, action_seed=7, action_tick0=100, **rec)
            env.Sync()
            return {k: forms.host(v) for k, v in rec.items()}
    whole, first, second = run(n1 + n2, 0), run(n1, 0), run(n2, n1)
    for k in ("rec_actions", "rec_obs", "rec_done"):
        assert np.array_equal(whole[k][..., :n1].view(np.uint8), first[k].view(np.uint8)), k
        assert np.array_equal(whole[k][..., n1:].view(np.uint8), second[k].view(np.uint8)), k
    assert whole["rec_done"].any() and len(np.unique(whole["rec_actions"])) == 2
