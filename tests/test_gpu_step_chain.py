"""The headline step kernel's shortened chain (docs/ledger.md §38; csrc/step_kernels.hpp step_kernel / pre_all_late_done, csrc/envs.hpp
CartPole::done_terms_filter): the done flags come from float32 compares unless some sub-lane of the wave is within four ulps of a threshold
(or holds a NaN), in which case the whole wave takes the binary64 compares; the workgroup's first lane is one unsigned 32 x 32 -> 64 scalar
multiply, the full-workgroup guard a scalar compare, and the next tick is written behind the body.  Nothing a caller sees may change.

  kernel    step_kernel<CartPole,4,true,false,15,1>, forced by SetLaunchPolicy(vec=4, nt=15, block=256, reset_form=1)
  lanes     1024 (one full workgroup), 2048 (two), 1027 (a full workgroup and a guarded tail), 3 (the tail alone)
  offsets   lane offset 0 and 2^32 + 5 (the Philox counter's lane word carries into its high half)
  states    draw / fin1 / fin64 / fin65: 0, 1, 64, 65 finished sub-lanes in the first wave (asserted from the oracle's step 0);
            band: in the first wave, positions at exactly +-threshold and 1 and 2 float32 steps either side of it (velocity 0, so the sum is
            the position), for both thresholds, and the 22 reference-text vectors whose flag a float32 compare flips — every other wave
            holds the reset draw's range, so the binary64 side is taken by some waves and not by others (asserted from the band's
            constants: a condition on the start state, the kernel's route is not observable);
            nonfinite: NaN in x_dot in one wave, +inf in theta_dot in another
  paths     StepDevice for 16 steps, RolloutDevice eager, RolloutDevice replaying a hipGraph
References, bit for bit: the oracle's float32 auto-reset vector step at every step (state, reward, done, tick; computed once per case and
shared by the paths) and a handle of the scalar form (vec 1, reset form 0)."""
import os

import numpy as np
import pytest

SEED, STEPS, BLOCK, VEC = 0x5EED, 16, 256, 4
GYM = "CartPole-v1"
HEADLINE = "step_kernel<CartPole,4,true,false,15,1>"
WAVE = 64 * VEC
SIZES = (BLOCK * VEC, 2 * BLOCK * VEC, BLOCK * VEC + 3, 3)
STATES = ("draw", "fin1", "fin64", "fin65", "band", "nonfinite")
OFFSETS = (0, (1 << 32) + 5)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X_THR, THETA_THR, TAU = np.float32(2.4), np.float32(0.20943951606750488), np.float32(0.02)


def _eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _steps(f, d):
    """d float32 steps from a positive f, away from zero for d > 0"""
    return (np.array([f], np.float32).view(np.uint32) + np.uint32(d & 0xFFFFFFFF)).view(np.float32)[0]


def _ambiguous(s):
    """per lane: the pre-filter leaves a term to the binary64 compares (csrc/cartpole_done_filter.hpp: four steps either side, NaN)"""
    out = np.zeros(s.shape[1], bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for p0, p1, thr in ((s[0], s[1], X_THR), (s[2], s[3], THETA_THR)):
            lo, hi = _steps(thr, -4), _steps(thr, 4)
            w = np.abs(p0 + TAU * p1)
            out |= ~((np.abs(p0) < lo) & ((w < lo) | (w > hi)))
    return out


def _flipping_vectors():
    g = np.load(os.path.join(ROOT, "tests", "golden", "cartpole_reference_text.npz"))
    s = g["state"].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        naive = (np.abs(s[0] + TAU * s[1]) > X_THR) | (np.abs(s[2] + TAU * s[3]) > THETA_THR)
    v = s[:, naive != g["done"].astype(bool)]
    assert v.shape[1] == 22, v.shape
    return v


def _start(n, case, rng):
    """([4, n] float32 start state, finished sub-lanes of the first wave at step 0 or None where the case does not fix them)"""
    wave = min(n, WAVE)
    s = rng.uniform(-0.05, 0.05, (4, n)).astype(np.float32)
    if case in ("draw", "fin1", "fin64", "fin65"):
        count = min({"draw": 0, "fin1": 1, "fin64": 64, "fin65": 65}[case], wave)
        fin = np.zeros(n, bool)
        fin[rng.permutation(wave)[:count]] = True
        if count:
            fin[wave:] = rng.random(n - wave) < 0.25
        k = int(fin.sum())
        side = np.where(rng.random(k) < 0.5, -1.0, 1.0)
        s[:, fin] = np.stack([rng.uniform(-1, 1, k), rng.uniform(-1, 1, k), 0.2 * side, 3.0 * side]).astype(np.float32)   # past the threshold
        return s, count
    if case == "band":
        special = []
        for row, thr in ((0, X_THR), (2, THETA_THR)):
            for sign in (-1.0, 1.0):
                for d in (0, -1, 1, -2, 2):
                    v = rng.uniform(-0.05, 0.05, 4).astype(np.float32)
                    v[row], v[row + 1] = np.float32(sign) * _steps(thr, d), 0.0
                    special.append(v)
        special = np.concatenate([np.stack(special, axis=1), _flipping_vectors()], axis=1)           # 20 + 22 vectors
        lanes = rng.permutation(wave)[:min(wave, special.shape[1])]
        s[:, lanes] = special[:, rng.permutation(special.shape[1])[:len(lanes)]]
        amb = _ambiguous(s)
        waves = [amb[i:i + WAVE].any() for i in range(0, n, WAVE)]
        assert waves[0] and (len(waves) == 1 or not any(waves[1:])), waves       # the binary64 side in the first wave, the float32 side elsewhere
        return s, None
    assert case == "nonfinite"
    s[1, 5 % n] = np.nan                                   # x + tau * NaN = NaN: every compare is false, the lane never finishes
    s[3, (WAVE + 9) % n] = np.inf                          # theta + tau * inf = inf: finishes
    return s, None


def _ring(n, stride, rng):
    acts = np.zeros((STEPS, stride), np.int32)
    lane = np.arange(n)
    for t in range(STEPS):
        acts[t, :n] = (((lane // VEC) + 5 * t) % 16 >> (lane % VEC)) & 1
    return acts


def _open(gpu_pkg, n, lane_offset, path, **policy):
    env = gpu_pkg.VectorEnv(GYM, n, seed=SEED, auto_reset=True, dtype=np.float32, lane_offset=lane_offset)
    env.SetLaunchPolicy(graph=1 if path == "graph" else 0, **policy)
    return env


def _snapshot(env):
    env.Sync()
    out = env.Read()
    return env.GetState(), out.Reward.copy(), env.GetArray("done").copy()


@pytest.mark.gpu
@pytest.mark.parametrize("lane_offset", OFFSETS)
@pytest.mark.parametrize("case", STATES)
@pytest.mark.parametrize("n", SIZES)
def test_shortened_chain_equals_the_oracle_and_the_scalar_form(gpu_pkg, oracle, n, case, lane_offset):
    import torch
    rng = np.random.default_rng(n * 131 + STATES.index(case) * 7 + lane_offset % 1009)
    s0, count = _start(n, case, rng)
    stride = (n + 63) // 64 * 64                 # every action slice 16-byte aligned
    acts = _ring(n, stride, rng)
    ring = torch.from_numpy(acts).cuda()
    torch.cuda.synchronize()                     # the handle launches on a stream of its own

    wide = dict(vec=VEC, nt=15, block=BLOCK, reset_form=1)
    with _open(gpu_pkg, n, lane_offset, "step", **wide) as env, _open(gpu_pkg, n, lane_offset, "step", vec=1, sequential_lanes=1, reset_form=0) as ref:
        assert env.KernelName() == HEADLINE, env.KernelName()
        assert ref.KernelName().startswith("step_kernel<CartPole,1,true,false,"), ref.KernelName()
        for e in (env, ref):
            e.ResetDevice()
            e.SetState(s0)
        tick0 = env.Tick
        assert ref.Tick == tick0
        trace, s = [], s0                        # the oracle's replay, once: state / reward / done after every step
        for t in range(STEPS):
            s, _, rw, dn = oracle.env_autoreset_step(GYM, SEED, lane_offset, tick0 + t, s, acts[t, :n])
            trace.append((s, rw, dn))
        fin0 = int(trace[0][2][:WAVE].astype(bool).sum())
        print(f"n {n} {case} offset {lane_offset}: first wave finishes {fin0} sub-lanes at step 0, the batch {int(trace[0][2].astype(bool).sum())}")
        if count is not None:
            assert fin0 == count, (fin0, count)                      # the start state does what it is built for, on THESE actions
        if case == "band" and n >= WAVE:
            assert 0 < fin0 < WAVE                                   # some of the near-threshold sub-lanes finish, some do not (3 lanes: whichever 3 vectors were drawn)
        if case == "nonfinite":
            assert not trace[0][2][5 % n] and trace[0][2][(WAVE + 9) % n] and np.isnan(trace[0][0][:, 5 % n]).any()
        for t in range(STEPS):
            env.StepDevice(ring[t])
            ref.StepDevice(ring[t])
            got, want = _snapshot(env), _snapshot(ref)
            for name, g, w, o in zip(("state", "reward", "done"), got, want, trace[t]):
                assert _eq(g, o), (t, name, "oracle")
                assert _eq(g, w), (t, name, "scalar form")
        assert env.Tick - tick0 == STEPS and ref.Tick - tick0 == STEPS

    for path in ("rollout", "graph"):
        with _open(gpu_pkg, n, lane_offset, path, **wide) as env:
            assert env.KernelName() == HEADLINE, env.KernelName()
            env.ResetDevice()
            env.SetState(s0)
            assert env.Tick == tick0
            env.RolloutDevice(ring, STEPS, stride, STEPS)
            got = _snapshot(env)
            for name, g, o in zip(("state", "reward", "done"), got, trace[-1]):
                assert _eq(g, o), (path, name)
            assert env.Tick - tick0 == STEPS, path


def test_band_start_state_reaches_both_sides_of_the_filter():
    """CPU only: the `band` start states hold what they name — ambiguous sub-lanes in the first wave only, the exact thresholds, their
    neighbours and the 22 flipping vectors among them."""
    for n in SIZES:
        s, _ = _start(n, "band", np.random.default_rng(n))
        amb = _ambiguous(s)
        assert amb[:WAVE].any() and not amb[WAVE:].any()
        if n >= WAVE:
            assert int(amb.sum()) >= 42 - 4          # (a few of the 42 special vectors may be decided: two steps outside a threshold with a velocity away from it)
            assert (np.abs(s[0]) == X_THR).sum() == 2 and (np.abs(s[2]) == THETA_THR).sum() >= 2
