"""tests/golden/make_mountaincar_continuous_golden.py — regenerates tests/golden/mountaincar_continuous.npz.

PROVENANCE: MountainCarContinuous-v0 is absent from the reference (README.md:69-76); the spec is upstream gym's
continuous_mountain_car.py, restated in float64 by tests/_mountaincar_continuous_twin.py step_f64.  The fixture is data: float32 start
states and actions (what the GPU is handed) and the float64 restatement's next state, reward and done flag for each — teacher-forced, one
step from each recorded state.  The states cover the velocity clip at +-0.07, the left wall (p = -1.2 with v < 0 zeroes v), the right
clip at 0.6, the goal (p >= 0.45 with v >= 0, both sides of the float32 threshold) and float32 states of energy-pumping trajectories;
the actions include the bounds, -0.0 and out-of-range values (the clamp feeds the force, the raw action the reward).

Run:  python tests/golden/make_mountaincar_continuous_golden.py      (deterministic)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _mountaincar_continuous_twin as tw  # noqa: E402

f32 = np.float32


def states(rng):
    parts = []
    n = 1500                                                              # the whole observation box
    parts.append(np.stack([rng.uniform(-1.2, 0.6, n), rng.uniform(-0.07, 0.07, n)]))
    n = 300                                                               # velocity clip: |v| near 0.07, pushed further
    side = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    parts.append(np.stack([rng.uniform(-1.0, 0.3, n), side * rng.uniform(0.0685, 0.07, n)]))
    n = 300                                                               # the left wall
    parts.append(np.stack([rng.uniform(-1.2, -1.13, n), rng.uniform(-0.07, 0.005, n)]))
    parts.append(np.stack([np.full(20, -1.2), rng.uniform(-0.07, 0.0, 20)]))
    n = 100                                                               # the right clip
    parts.append(np.stack([rng.uniform(0.55, 0.6, n), rng.uniform(0.0, 0.07, n)]))
    n = 800                                                               # the goal
    parts.append(np.stack([rng.uniform(0.38, 0.46, n), rng.uniform(-0.01, 0.07, n)]))
    n = 60                                                                # at the threshold itself (v >= 0: p stays, or moves a little)
    parts.append(np.stack([np.where(rng.random(n) < 0.5, tw.GOAL32, tw.BELOW_GOAL32), rng.choice([0.0, 1e-7, 1e-3], n)]))
    # energy-pumping trajectories (a = sign(v)), float64 dynamics, stored as float32
    lanes, steps = 8, 160
    s = np.stack([rng.uniform(-0.6, -0.4, lanes), np.zeros(lanes)])
    traj = []
    for _ in range(steps):
        s = s.astype(f32).astype(np.float64)
        traj.append(s.copy())
        s, _, _ = tw.step_f64(s, np.where(s[1] >= 0, 1.0, -1.0))
    parts.append(np.concatenate(traj, axis=1))
    return np.concatenate(parts, axis=1).astype(f32)


def actions(rng, n):
    a = rng.uniform(-1.0, 1.0, n)
    pick = rng.random(n)
    a[pick < 0.05] = 1.0
    a[(pick >= 0.05) & (pick < 0.10)] = -1.0
    a[(pick >= 0.10) & (pick < 0.13)] = 0.0
    a[(pick >= 0.13) & (pick < 0.15)] = -0.0
    far = pick >= 0.85                                                   # out of range: clamped for the force, raw in the reward
    a[far] = rng.choice([-1e3, -50.0, -3.0, -1.5, -1.0000001, 1.0000001, 1.5, 3.0, 50.0, 1e3], far.sum())
    return a.astype(f32)


def main():
    rng = np.random.default_rng(20261016)
    s = states(rng)
    a = actions(rng, s.shape[1])
    a[-1280:] = np.where(s[1, -1280:] >= 0, 1.0, -1.0)                  # the trajectories' own actions
    ns, rw, done = tw.step_f64(s.astype(np.float64), a.astype(np.float64))
    np.savez_compressed(os.path.join(HERE, "mountaincar_continuous.npz"), state=s, action=a, next_state=ns, reward=rw,
                        done=done.astype(np.uint8))
    print("mountaincar_continuous.npz:", s.shape[1], "states,", int(done.sum()), "terminal")


if __name__ == "__main__":
    main()
