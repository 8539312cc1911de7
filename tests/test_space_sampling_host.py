"""CPU tests of the space-sampling reference (tests/_space_sampling_ref.py) and of the oracle's bounded Box draw.

The float64 / integer reference the GPU tests hold the kernels against is itself held against the C oracle wherever the two state
the same thing; the lanes with extreme Philox words that the helper commits are re-derived from the oracle; and the oracle's
bounded draw — the kernel's bit-twin — must stay finite and inside bounds as wide as CartPole's own ObservationSpace
(+-float.MaxValue velocities, CartPoleEnv.cs:46-48), where `high - low` overflows float32."""
import numpy as np
import pytest

import _space_sampling_ref as R

SEED, TICK, COUNT = 0x5EED, 9, 1029
LANE_OFFSETS = [0, 1, 2, 3, (1 << 34) - 6, (1 << 33) + 3]     # 2^34 - 6: the group counter's low word wraps inside the batch
FMAX = R.FLT_MAX


@pytest.mark.parametrize("lane0", LANE_OFFSETS)
def test_integer_reference_equals_the_oracle(oracle, lane0):
    a, b = R.words(oracle, SEED, lane0, TICK, COUNT)
    rng = np.random.default_rng(lane0 & 0xFFFF)
    for n in (1, 2, 3, 37, (1 << 31) - 1):
        for start in (0, 10, -5):
            assert np.array_equal(R.discrete_sample(a, n, start), oracle.discrete_sample(SEED, lane0, TICK, n, start, COUNT)), (n, start)
    for n in (3, 37):
        rows = rng.choice(np.array([0, 1, 1, 2, 255], np.uint8), size=(COUNT, n))
        rows[::7] = 0                                                   # no valid action -> start
        rows[3::7] = 2
        rows[5::7] = 0
        rows[5::7, n - 1] = 1                                           # one valid action
        assert np.array_equal(R.discrete_sample_masked(a, rows, n, 10), oracle.discrete_sample_masked(SEED, lane0, TICK, n, 10, rows, COUNT))
        for shared in (rows[1], rows[0], rows[5]):
            assert np.array_equal(R.discrete_sample_masked(a, shared, n, -5), oracle.discrete_sample_masked(SEED, lane0, TICK, n, -5, shared, COUNT))
    coin = float(np.float32((int(b[17]) >> 8) / R.TWO24))              # a lane's own coin, and the float just below it
    for n in (2, 3):
        policy = rng.integers(0, n, COUNT).astype(np.int32)
        for eps in (0.0, 0.25, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -24, coin, float(np.nextafter(np.float32(coin), np.float32(0)))):
            assert np.array_equal(R.compose_discrete(a, b, n, eps, policy), oracle.compose_discrete(SEED, lane0, TICK, n, eps, policy)), (n, eps)


# Bounds for which the oracle's float32 form low + (high - low) * u rounds at most once: low == 0 (the sum is exact and so is the
# width), or a width 2^k around zero ((high - low) * u and the sum are both exact).  Only there can a float32 result lie within
# HALF a spacing of the exact value everywhere.
SINGLE_ROUNDING_BOUNDS = [(0.0, 4.8), (0.0, 0.3), (0.0, FMAX), (-1.0, 1.0), (-2.0, 2.0)]
# Any other bounds round three times (width, product, sum), and a draw next to zero can then be many of its OWN spacings from the
# exact value ((-5, 5): the product carries half a spacing of 10).  Bound: the three roundings added up.
THREE_ROUNDING_BOUNDS = [(-5.0, 5.0), (0.1, 0.3), (-1.0, 1e-3), (-4.8, 4.8)]


@pytest.mark.parametrize("lane0", LANE_OFFSETS)
def test_bounded_reference_is_within_half_a_spacing_of_the_oracle(oracle, lane0):
    a, b = R.words(oracle, SEED, lane0, TICK, COUNT)
    u = R.uniforms(a, b)[0]
    for low, high in SINGLE_ROUNDING_BOUNDS:
        got = oracle.box_uniform_sample(SEED, lane0, TICK, low, high, COUNT)
        ref = R.box_sample(low, high, a, b)
        assert (np.abs(got.astype(np.float64) - ref) <= 0.5 * np.spacing(np.abs(got)).astype(np.float64)).all(), (low, high)
    for low, high in THREE_ROUNDING_BOUNDS:
        got = oracle.box_uniform_sample(SEED, lane0, TICK, low, high, COUNT)
        ref = R.box_sample(low, high, a, b)
        width = np.float32(high) - np.float32(low)
        bound = 0.5 * (float(np.spacing(width)) * u + np.spacing(np.abs(width * u.astype(np.float32))).astype(np.float64)
                       + np.spacing(np.abs(got)).astype(np.float64))
        assert (np.abs(got.astype(np.float64) - ref) <= bound).all(), (low, high)


def test_committed_extreme_lanes_carry_the_words_they_claim(oracle):
    ln2_24 = 24.0 * np.log(2.0)
    for kind, lanes, word, top in (("A_ZERO", R.A_ZERO, 0, 0), ("A_MAX", R.A_MAX, 0, 0xFFFFFF), ("B_ZERO", R.B_ZERO, 1, 0), ("B_MAX", R.B_MAX, 1, 0xFFFFFF)):
        assert len(lanes) >= 2 and len(set(lanes)) == len(lanes)
        for lane in lanes:
            w = oracle.action_words(R.EXTREME_SEED, lane, R.EXTREME_TICK, 1)
            assert int(w[word][0]) >> 8 == top, (kind, lane)
    assert {first + R.WINDOW_LEAD for first, _ in R.extreme_windows()} == set(R.A_ZERO + R.A_MAX + R.B_ZERO + R.B_MAX)
    assert all(first >= 0 and first <= lane < first + R.WINDOW for first, lane in R.extreme_windows())
    # what the reference makes of them: u == 0 is exactly the finite bound, the largest u is bound + 24 ln 2, the smallest u1 finite
    for lane in R.A_ZERO:
        a, b = R.words(oracle, R.EXTREME_SEED, lane, R.EXTREME_TICK, 1)
        assert R.box_sample(2.0, np.inf, a, b)[0] == 2.0 and R.box_sample(-np.inf, 7.0, a, b)[0] == 7.0 and R.box_sample(-FMAX, FMAX, a, b)[0] == -FMAX
        g = R.box_sample(-np.inf, np.inf, a, b)[0]
        assert np.isfinite(g) and abs(g - 0.5) <= np.sqrt(48.0 * np.log(2.0))
    for lane in R.A_MAX:
        a, b = R.words(oracle, R.EXTREME_SEED, lane, R.EXTREME_TICK, 1)
        assert abs(R.box_sample(2.0, np.inf, a, b)[0] - (2.0 + ln2_24)) < 1e-12 and abs(R.box_sample(-np.inf, 7.0, a, b)[0] - (7.0 + ln2_24)) < 1e-12
        assert R.box_sample(-np.inf, np.inf, a, b)[0] == 0.5             # u1 == 1: radius 0


@pytest.mark.parametrize("low,high", [(-FMAX, FMAX), (-FMAX, 4.8), (-3e38, 3e38)])
def test_oracle_bounded_draw_survives_bounds_wider_than_float32(oracle, low, high):
    """Before the convex form low * (1 - u) + high * u for an overflowing width, every draw of the first and the last of these was
    +inf (NaN at u == 0)."""
    low32, high32 = np.float32(low), np.float32(high)                   # (-FMAX, 4.8): the width rounds to FMAX and stays finite
    bound = R.wide_bounded_bound(low32, high32)
    batches = [(11, 1 << 16)] + [(first, R.WINDOW) for first, _ in R.extreme_windows()]
    for lane0, count in batches:
        got = oracle.box_uniform_sample(R.EXTREME_SEED, lane0, R.EXTREME_TICK, low, high, count)
        ref = R.box_sample(low, high, *R.words(oracle, R.EXTREME_SEED, lane0, R.EXTREME_TICK, count))
        assert np.isfinite(got).all(), (lane0, int((~np.isfinite(got)).sum()), count)
        assert (got >= low32).all() and (got <= high32).all(), lane0
        assert (np.abs(got.astype(np.float64) - ref) <= bound).all(), (lane0, np.abs(got.astype(np.float64) - ref).max(), bound)
    for lane in R.A_ZERO:                                                # u == 0 is exactly the lower bound
        assert oracle.box_uniform_sample(R.EXTREME_SEED, lane, R.EXTREME_TICK, low, high, 1)[0] == low32
