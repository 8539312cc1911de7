"""The full-workgroup body of the headline step kernel runs CartPole's step in the two parts the env cuts it into where the action enters
(csrc/envs.hpp CartPole::step_pre / step_post; csrc/step_kernels.hpp step_body_wg): the action-free part of the four sub-lanes, the done
flags and the reset's draw in front of the wait for the action, the rest behind it.  The two parts exchange eight values per sub-lane and
the action meets them late, so a mix-up of sub-lanes or threads between the halves is what can go wrong — and nothing else may change: the
results are the bits of the unsplit step.

  kernel    step_kernel<CartPole,4,true,false,15,1>, forced by SetLaunchPolicy(vec=4, nt=15, block=256, reset_form=1) at small sizes
  lanes     1024 (one full workgroup), 2048 (two), 1027 (a full workgroup and a guarded tail), 3 (the tail alone: the unsplit body)
  actions   "bits": thread i holds the four bits of (i + 5 t) mod 16 as its sub-lanes' actions at step t — all 16 patterns, a different
            slice of the ring every step; "wild": values outside {0, 1} (2, -1, 0x7fffffff), which push left like 0
  states    the reset draw's own range (nothing finishes at step 0); exactly 1, 64 and 65 finished sub-lanes in the first wave (the single
            trip, its boundary, the round loop behind it) with about a quarter of the lanes behind it finishing; every lane finished; one
            lane with |theta| = 1.0 (its wave takes the general trigonometry, every other wave the small-angle path); one lane with NaN
            and one with +inf in theta_dot.  The finish counts are asserted per case from the oracle's step 0
  paths     StepDevice per step, RolloutDevice eager, RolloutDevice replaying a hipGraph
References, bit for bit over 16 consecutive steps: the oracle's float32 auto-reset vector step (ref_env_autoreset_step_batch_f32, computed
once per case and shared by the paths) for state, reward, done and the tick, and a handle of the scalar form (vec 1, reset form 0)."""
import numpy as np
import pytest

SEED, STEPS, BLOCK, VEC = 0x5EED, 16, 256, 4
GYM = "CartPole-v1"
HEADLINE = "step_kernel<CartPole,4,true,false,15,1>"
WAVE = 64 * VEC                                  # lanes of one wave of the wide form
SIZES = (BLOCK * VEC, 2 * BLOCK * VEC, BLOCK * VEC + 3, 3)
STATES = ("draw", "fin1", "fin64", "fin65", "all", "general", "nonfinite")
ACTIONS = ("bits", "wild")
PATHS = ("step", "rollout", "graph")


def _eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _start(n, case, rng):
    """([4, n] float32 start state, sub-lanes of the first wave that finish at step 0)"""
    wave = min(n, WAVE)
    s = rng.uniform(-0.05, 0.05, (4, n))
    fin = np.zeros(n, bool)
    count = {"draw": 0, "fin1": 1, "fin64": 64, "fin65": 65, "all": wave, "general": 1, "nonfinite": 1}[case]
    count = min(count, wave)
    if case in ("fin1", "fin64", "fin65"):
        fin[rng.permutation(wave)[:count]] = True
        fin[wave:] = rng.random(n - wave) < 0.25
    elif case == "all":
        fin[:] = True
    k = int(fin.sum())
    side = np.where(rng.random(k) < 0.5, -1.0, 1.0)
    s[:, fin] = np.stack([rng.uniform(-1, 1, k), rng.uniform(-1, 1, k), 0.2 * side, 3.0 * side])   # past the threshold whatever the push
    if case == "general":
        s[2, 5 % n] = -1.0                       # beyond kSmallAngle (and beyond the threshold: the lane finishes, in the general path)
    if case == "nonfinite":
        s[3, 5 % n] = np.nan                     # NaN: every compare is false — the lane never finishes
        s[3, 9 % n] = np.inf                     # theta + tau * inf = inf: finishes
    return s.astype(np.float32), count


def _ring(n, stride, kind, rng):
    acts = np.zeros((STEPS, stride), np.int32)
    lane = np.arange(n)
    for t in range(STEPS):
        if kind == "bits":
            acts[t, :n] = (((lane // VEC) + 5 * t) % 16 >> (lane % VEC)) & 1
        else:
            acts[t, :n] = rng.choice(np.array([2, -1, 0x7fffffff, 0, 1], np.int32), n)
    return acts


def _open(gpu_pkg, n, path, **policy):
    env = gpu_pkg.VectorEnv(GYM, n, seed=SEED, auto_reset=True, dtype=np.float32)
    env.SetLaunchPolicy(graph=1 if path == "graph" else 0, **policy)
    return env


def _snapshot(env):
    env.Sync()
    out = env.Read()
    return env.GetState(), out.Reward.copy(), env.GetArray("done").copy()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ACTIONS)
@pytest.mark.parametrize("case", STATES)
@pytest.mark.parametrize("n", SIZES)
def test_split_step_equals_the_oracle_and_the_scalar_form(gpu_pkg, oracle, n, case, kind):
    import torch
    rng = np.random.default_rng(n * 131 + STATES.index(case) * 7 + ACTIONS.index(kind))
    s0, count = _start(n, case, rng)
    stride = (n + 63) // 64 * 64                 # every action slice 16-byte aligned
    acts = _ring(n, stride, kind, rng)
    if kind == "bits":
        assert len({tuple(acts[0, 4 * i:4 * i + 4]) for i in range(n // 4)}) == min(16, n // 4)   # every pattern of four
    else:
        seen = set(np.unique(acts[:, :n]).tolist())
        assert seen <= {-1, 0, 1, 2, 0x7fffffff} and (n < WAVE or len(seen) == 5)
        pushed = oracle.env_autoreset_step(GYM, SEED, 0, 1, s0, acts[0, :n])[0]
        as_zero = oracle.env_autoreset_step(GYM, SEED, 0, 1, s0, np.where(acts[0, :n] == 1, 1, 0).astype(np.int32))[0]
        assert _eq(pushed, as_zero)              # anything but 1 pushes left
    ring = torch.from_numpy(acts).cuda()
    torch.cuda.synchronize()                     # the handle launches on a stream of its own

    wide = dict(vec=VEC, nt=15, block=BLOCK, reset_form=1)
    with _open(gpu_pkg, n, "step", **wide) as env, _open(gpu_pkg, n, "step", vec=1, sequential_lanes=1, reset_form=0) as ref:
        assert env.KernelName() == HEADLINE, env.KernelName()
        assert ref.KernelName().startswith("step_kernel<CartPole,1,true,false,"), ref.KernelName()
        for e in (env, ref):
            e.ResetDevice()
            e.SetState(s0)
        tick0 = env.Tick
        assert ref.Tick == tick0
        # the oracle's replay, once: state / reward / done after every step
        trace, s = [], s0
        for t in range(STEPS):
            s, _, rw, dn = oracle.env_autoreset_step(GYM, SEED, 0, tick0 + t, s, acts[t, :n])
            trace.append((s, rw, dn))
        fin0 = int(trace[0][2][:WAVE].astype(bool).sum())
        print(f"n {n} {case} {kind}: first wave finishes {fin0} sub-lanes at step 0, the batch {int(trace[0][2].astype(bool).sum())}")
        assert fin0 == count, (fin0, count)                          # the start state does what it is built for, on THESE actions
        if case == "all":
            assert trace[0][2].all()
        if case == "nonfinite":
            assert not trace[0][2][5 % n] and trace[0][2][9 % n] and np.isnan(trace[0][0][:, 5 % n]).any()
        for t in range(STEPS):
            env.StepDevice(ring[t])
            ref.StepDevice(ring[t])
            got, want = _snapshot(env), _snapshot(ref)
            for name, g, w, o in zip(("state", "reward", "done"), got, want, trace[t]):
                assert _eq(g, o), (t, name, "oracle")
                assert _eq(g, w), (t, name, "scalar form")
        assert env.Tick - tick0 == STEPS and ref.Tick - tick0 == STEPS

    for path in PATHS[1:]:
        with _open(gpu_pkg, n, path, **wide) as env:
            assert env.KernelName() == HEADLINE, env.KernelName()
            env.ResetDevice()
            env.SetState(s0)
            assert env.Tick == tick0
            env.RolloutDevice(ring, STEPS, stride, STEPS)
            got = _snapshot(env)
            for name, g, o in zip(("state", "reward", "done"), got, trace[-1]):
                assert _eq(g, o), (path, name)
            assert env.Tick - tick0 == STEPS, path
