"""GPU tests of the stand-alone space samplers (csrc/kernels.hip: sample_box_kernel, sample_box_elementwise_kernel,
sample_discrete_kernel, sample_discrete_masked_kernel, compose_discrete_kernel) against the per-element float64 / integer
reference of tests/_space_sampling_ref.py: every count, lane-offset residue and output misalignment `store_group` distinguishes,
with sentinels around the output; every Box regime element by element, at the lanes whose Philox words are extreme too; bounds as
wide as float32; masks with padding; an epsilon that equals a lane's coin."""
import ctypes as C

import numpy as np
import pytest

import _space_sampling_ref as R

pytestmark = pytest.mark.gpu

SEED, TICK = 0x5EED, 9
INF = float("inf")
FMAX = R.FLT_MAX
SENTINEL = -0x21524111                       # 0xDEADBEEF as int32; as float32 bits a value no sampler returns
MARGIN = 64                                  # int32 words kept around every output: 256 bytes on each side
COUNTS = [1, 2, 3, 4, 5, 7, 1021, 1024, 1025, 2 * 1024 + 4 * 37 + 3]
BIG_LANE_OFFSETS = [(1 << 34) - 6, (1 << 33) + 3]     # the group counter's low word wraps inside the batch; a high word alone


class Guarded:
    """`count` 4-byte elements at base + 256 + byte_offset of a sentinel-filled allocation whose base is 256-byte aligned."""

    def __init__(self, torch, count, byte_offset=0):
        assert byte_offset % 4 == 0
        self.torch, self.count, self.first = torch, count, MARGIN + byte_offset // 4
        self.raw = torch.full((MARGIN + count + MARGIN + 4,), SENTINEL, dtype=torch.int32, device="cuda")
        assert self.raw.data_ptr() % 256 == 0
        self.ptr = self.raw.data_ptr() + 4 * self.first
        torch.cuda.synchronize()

    def check(self, want, what):
        """Elements [0, count) equal `want` bit for bit and every other byte of the allocation still holds the sentinel."""
        self.torch.cuda.synchronize()
        got = self.raw.cpu().numpy()
        full = np.full(got.shape, SENTINEL, np.int32)
        full[self.first:self.first + self.count] = np.ascontiguousarray(want).view(np.int32)
        stray = np.nonzero(got != full)[0] - self.first
        assert stray.size == 0, (what, "first differing elements (index relative to the output):", stray[:8].tolist())

    def values(self, dtype):
        """The output as `dtype`, after checking that nothing outside it was written."""
        self.torch.cuda.synchronize()
        got = self.raw.cpu().numpy()
        outside = np.concatenate([got[:self.first], got[self.first + self.count:]])
        assert (outside == SENTINEL).all(), "a store outside the output"
        return got[self.first:self.first + self.count].view(dtype).copy()


@pytest.fixture(scope="module")
def api(gpu_pkg):
    import torch
    return torch, gpu_pkg.load_library(), gpu_pkg._capi


def _box(api, out, count, low, high, seed, lane_offset, tick):
    _, lib, capi = api
    capi.check(lib.gymnet_sample_box_device(0, None, C.c_void_p(out.ptr), count, low, high, seed, lane_offset, tick))


def _discrete(api, out, count, n, start, seed, lane_offset, tick):
    _, lib, capi = api
    capi.check(lib.gymnet_sample_discrete_device(0, None, C.c_void_p(out.ptr), count, n, start, seed, lane_offset, tick))


@pytest.mark.parametrize("kernel", ["discrete", "box"])
def test_every_count_lane_residue_and_output_alignment(api, oracle, kernel):
    """store_group leaves a whole in-batch group on a 16-byte aligned address as one dwordx4 store and everything else element by
    element: all 16 combinations of (lane_offset & 3, byte misalignment of out) at counts from 1 to several workgroups."""
    torch = api[0]

    def run(count, lane_offset, byte_offset):
        out = Guarded(torch, count, byte_offset)
        if kernel == "discrete":
            _discrete(api, out, count, 37, 10, SEED, lane_offset, TICK)
            want = R.discrete_sample(R.words(oracle, SEED, lane_offset, TICK, count)[0], 37, 10) if count else np.zeros(0, np.int32)
            if count:
                assert np.array_equal(want, oracle.discrete_sample(SEED, lane_offset, TICK, 37, 10, count))
        else:
            _box(api, out, count, -5.0, 5.0, SEED, lane_offset, TICK)
            want = oracle.box_uniform_sample(SEED, lane_offset, TICK, -5.0, 5.0, count)
        out.check(want, (kernel, count, lane_offset, byte_offset))

    for count in COUNTS:
        for residue in range(4):
            for byte_offset in (0, 4, 8, 12):
                run(count, 4100 + residue, byte_offset)
    for lane_offset in BIG_LANE_OFFSETS:
        run(1025, lane_offset, 4)
    run(0, 4101, 0)                                                      # count == 0: OK, and nothing written


def test_handle_bound_forms_use_the_handles_own_count_and_offset(api, gpu_pkg, oracle):
    """SampleActionsDevice / SampleActionsMaskedDevice on a handle created with lane_offset = 4102 and an odd n, writing row 1 of a
    [3][n] ring (n * 4 bytes is no multiple of 16: the row starts misaligned); rows 0 and 2 keep their sentinel."""
    torch = api[0]
    n, off = 4099, 4102
    for name, nvals in (("CartPole-v1", 2), ("Acrobot-v1", 3)):
        with gpu_pkg.VectorEnv(name, n, seed=1, lane_offset=off) as env:
            ring = Guarded(torch, 3 * n)
            env.SampleActionsDevice(ring.ptr + 4 * n, seed=SEED, tick=TICK); env.Sync()
            a, _ = R.words(oracle, SEED, off, TICK, n)
            want = np.full(3 * n, SENTINEL, np.int32)
            want[n:2 * n] = R.discrete_sample(a, nvals, 0)
            ring.check(want, name)
            rng = np.random.default_rng(nvals)
            rows = rng.integers(0, 2, (n, nvals)).astype(np.uint8)
            rows[::5] = 0
            mask = torch.from_numpy(rows).cuda()
            ring = Guarded(torch, 3 * n)
            env.SampleActionsMaskedDevice(ring.ptr + 4 * n, mask, per_lane=True, seed=SEED, tick=TICK); env.Sync()
            want[n:2 * n] = R.discrete_sample_masked(a, rows, nvals, 0)
            ring.check(want, name + " masked")
    with gpu_pkg.VectorEnv("Pendulum-v1", n, seed=1, lane_offset=off) as env:      # Box action space: uniform(-2, 2)
        ring = Guarded(torch, 3 * n)
        env.SampleActionsDevice(ring.ptr + 4 * n, seed=SEED, tick=TICK); env.Sync()
        want = np.full(3 * n, SENTINEL, np.int32)
        want[n:2 * n] = oracle.box_uniform_sample(SEED, off, TICK, -2.0, 2.0, n).view(np.int32)
        ring.check(want, "Pendulum-v1")


def _extreme_batches(count=1 << 16):
    return [(11, count)] + [(first, R.WINDOW) for first, _ in R.extreme_windows()]


@pytest.mark.parametrize("low,high", [(2.0, INF), (-INF, 7.0), (-INF, INF)])
def test_unbounded_box_regimes_per_element(api, oracle, low, high):
    """The low-bounded, high-bounded and unbounded draws (Box.cs:82-84) element by element against the float64 reference, on 2^16
    lanes and on 8-lane windows around the lanes whose words are extreme.  Bounds (tests/_space_sampling_ref.py): one-sided
    4 * spacing(float32(max(|ln(1 - u)|, |result|))); unbounded 1e-5 absolute.
    Worst measured on the MI355X: (2, inf) 1.28e-6, 0.38 of the bound; (-inf, 7) 2.03e-6, 0.34 of the bound; (-inf, inf) 1.28e-6,
    0.13 of the bound."""
    torch = api[0]
    worst, worst_abs = 0.0, 0.0
    unbounded = low == -INF and high == INF
    finite_bound = low if low > -INF else high                           # (the unbounded regime has none)
    for lane0, count in _extreme_batches():
        out = Guarded(torch, count)
        _box(api, out, count, low, high, R.EXTREME_SEED, lane0, R.EXTREME_TICK)
        got = out.values(np.float32)
        a, b = R.words(oracle, R.EXTREME_SEED, lane0, R.EXTREME_TICK, count)
        ref = R.box_sample(low, high, a, b)
        err = np.abs(got.astype(np.float64) - ref)
        assert np.isfinite(got).all(), lane0
        bound = np.full(count, R.UNBOUNDED_BOUND) if unbounded else R.one_sided_bound(a, ref)
        worst, worst_abs = max(worst, (err / bound).max()), max(worst_abs, err.max())
        if not unbounded:
            assert (got >= np.float32(finite_bound)).all()                 # bound + Exp(1) never falls below its bound
        assert (err <= bound).all(), (lane0, int(np.argmax(err / bound)), err.max())
    print(f"box regime ({low}, {high}): worst |err| {worst_abs:.3e}, worst |err| / bound {worst:.3f}")
    # the extreme lanes themselves: u == 0 is exactly the finite bound; the largest u is the bound + 24 ln 2; the smallest u1 is finite
    for lane, expect in [(l, "zero") for l in R.A_ZERO] + [(l, "max") for l in R.A_MAX]:
        out = Guarded(torch, 1)
        _box(api, out, 1, low, high, R.EXTREME_SEED, lane, R.EXTREME_TICK)
        v = out.values(np.float32)[0]
        a, b = R.words(oracle, R.EXTREME_SEED, lane, R.EXTREME_TICK, 1)
        if unbounded:
            assert np.isfinite(v) and abs(float(v) - R.box_sample(low, high, a, b)[0]) <= R.UNBOUNDED_BOUND
        elif expect == "zero":
            assert v == np.float32(finite_bound)
        else:
            want = finite_bound + 24.0 * np.log(2.0)
            assert abs(float(v) - want) <= R.one_sided_bound(a, np.array([want]))[0]


ELEMENT_LOW = [-5.0, 2.0, -INF, -INF, -1.0, -FMAX, 0.1]
ELEMENT_HIGH = [5.0, INF, 7.0, INF, 1.0, FMAX, 0.3]


def _elementwise(api, out, count, low, high, seed, lane_offset, tick):
    torch, lib, capi = api
    lo = torch.tensor(low, dtype=torch.float32, device="cuda")
    hi = torch.tensor(high, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    capi.check(lib.gymnet_sample_box_elementwise_device(0, None, C.c_void_p(out.ptr), count, len(low), C.c_void_p(lo.data_ptr()),
                                                        C.c_void_p(hi.data_ptr()), seed, lane_offset, tick))
    torch.cuda.synchronize()


@pytest.mark.parametrize("count", [1, 3, 1000])
@pytest.mark.parametrize("lane_offset", [0, 3, (1 << 34) - 6])
def test_elementwise_sampler_draws_every_element_from_its_own_key(api, oracle, count, lane_offset):
    """Element e of every row against the reference computed from key seed + e * 0xD1B54A32D192ED03: the bounded elements carry the
    oracle's bit pattern at that key, the others lie within the regime bounds; sentinels before the first and after the last row."""
    torch, dim = api[0], len(ELEMENT_LOW)
    out = Guarded(torch, count * dim)
    _elementwise(api, out, count, ELEMENT_LOW, ELEMENT_HIGH, SEED, lane_offset, TICK)
    rows = out.values(np.float32).reshape(count, dim)
    assert np.isfinite(rows).all()
    for e, (low, high) in enumerate(zip(ELEMENT_LOW, ELEMENT_HIGH)):
        key = R.element_key(SEED, e)
        a, b = R.words(oracle, SEED, lane_offset, TICK, count, element=e)
        ref = R.box_sample(low, high, a, b)
        err = np.abs(rows[:, e].astype(np.float64) - ref)
        if low > -INF and high < INF:
            assert np.array_equal(rows[:, e].view(np.int32), oracle.box_uniform_sample(key, lane_offset, TICK, low, high, count).view(np.int32)), e
            assert (rows[:, e] >= np.float32(low)).all() and (rows[:, e] <= np.float32(high)).all(), e
            if high - low > FMAX:
                assert (err <= R.wide_bounded_bound(low, high)).all(), e
        elif low == -INF and high == INF:
            assert (err <= R.UNBOUNDED_BOUND).all(), (e, err.max())
        else:
            assert (err <= R.one_sided_bound(a, ref)).all(), (e, err.max())


def test_elementwise_sampler_on_cartpoles_own_observation_space(api, gpu_pkg, oracle):
    """ObservationSpace.Sample() for CartPole (CartPoleEnv.cs:46-48: velocities bounded by +-float.MaxValue, a width float32 cannot
    hold): every value finite, every row inside the space, on 2^16 rows and on rows at the lanes with extreme words — for element 0
    with the committed seed, and for the velocity element 1 with the seed that gives IT the committed key."""
    torch = api[0]
    with gpu_pkg.VectorEnv("CartPole-v1", 8) as env:
        space = env.ObservationSpace
    low, high = [float(v) for v in space.Low], [float(v) for v in space.High]
    assert low[1] == -FMAX and high[3] == FMAX
    seed_for_element_1 = (R.EXTREME_SEED - R.ELEMENT_KEY_STEP) & R.MASK64
    assert R.element_key(seed_for_element_1, 1) == R.EXTREME_SEED
    for seed, rows_in_bulk in ((R.EXTREME_SEED, 1 << 16), (seed_for_element_1, 1 << 10)):
        for lane0, count in _extreme_batches(rows_in_bulk):
            out = Guarded(torch, count * 4)
            _elementwise(api, out, count, low, high, seed, lane0, R.EXTREME_TICK)
            rows = out.values(np.float32).reshape(count, 4)
            assert np.isfinite(rows).all(), (seed, lane0, int((~np.isfinite(rows)).sum()))
            assert all(space.Contains(row) for row in rows), (seed, lane0)
            for e in (1, 3):                                             # the float.MaxValue elements, against the float64 reference
                ref = R.box_sample(low[e], high[e], *R.words(oracle, seed, lane0, R.EXTREME_TICK, count, element=e))
                assert (np.abs(rows[:, e].astype(np.float64) - ref) <= R.wide_bounded_bound(low[e], high[e])).all(), (seed, lane0, e)
    a_zero_row = Guarded(torch, 4)
    _elementwise(api, a_zero_row, 1, low, high, seed_for_element_1, R.A_ZERO[0], R.EXTREME_TICK)
    assert a_zero_row.values(np.float32)[1] == np.float32(-FMAX)         # u == 0 on a float.MaxValue element: exactly Low, not NaN


@pytest.mark.parametrize("low,high", [(0.1, 0.3), (-1.0, 1e-3), (-FMAX, FMAX), (-FMAX, 4.8), (5.0, 5.0), (-3e38, 3e38)])
def test_awkward_bounded_ranges(api, oracle, low, high):
    """Bounded draws whose bounds are no round numbers, degenerate, or as wide as float32: finite, inside [low, high], the oracle's
    bits; where high - low overflows, also within 2 spacings of the bound's magnitude of the float64 reference."""
    torch = api[0]
    low32, high32 = np.float32(low), np.float32(high)
    with np.errstate(over="ignore"):
        overflows = not np.isfinite(high32 - low32)
    for lane0, count in _extreme_batches():
        out = Guarded(torch, count)
        _box(api, out, count, low, high, R.EXTREME_SEED, lane0, R.EXTREME_TICK)
        got = out.values(np.float32)
        assert np.isfinite(got).all(), (lane0, int((~np.isfinite(got)).sum()))
        assert (got >= low32).all() and (got <= high32).all(), (lane0, got.min(), got.max())
        assert np.array_equal(got.view(np.int32), oracle.box_uniform_sample(R.EXTREME_SEED, lane0, R.EXTREME_TICK, low, high, count).view(np.int32)), lane0
        if overflows or max(abs(low), abs(high)) >= 1e38:
            ref = R.box_sample(low, high, *R.words(oracle, R.EXTREME_SEED, lane0, R.EXTREME_TICK, count))
            assert (np.abs(got.astype(np.float64) - ref) <= R.wide_bounded_bound(low, high)).all(), lane0


def test_discrete_sampler_matches_the_integer_reference(api, oracle):
    torch, count, lane_offset = api[0], 4096 + 3, 11
    a, _ = R.words(oracle, SEED, lane_offset, TICK, count)
    for n in (1, 2, 3, 37, (1 << 31) - 1):
        for start in (0, 10, -5):
            out = Guarded(torch, count)
            _discrete(api, out, count, n, start, SEED, lane_offset, TICK)
            out.check(R.discrete_sample(a, n, start), (n, start))
            if n == 1:
                assert (out.values(np.int32) == start).all()


def _mask_rows(rng, count, n, stride):
    rows = np.ones((count, stride), np.uint8)                            # padding bytes are 1: they must not count as valid actions
    rows[:, :n] = rng.choice(np.array([0, 1, 1, 2, 255], np.uint8), size=(count, n))
    rows[::7, :n] = 0                                                    # no valid action -> start
    rows[3::7, :n] = rng.choice(np.array([2, 255], np.uint8), size=rows[3::7, :n].shape)     # only bytes that are not 1 -> start
    rows[5::7, :n] = 0
    rows[5::7, n - 1] = 1                                                # exactly one valid action: the last
    return rows


@pytest.mark.parametrize("n", [3, 37])
def test_masked_sampler_rows_strides_and_edges(api, oracle, n):
    torch, lib, capi = api
    rng = np.random.default_rng(n)
    start = 10
    for count in (1, 3, 1025):
        for lane_offset in (4101, 4102):
            a, _ = R.words(oracle, SEED, lane_offset, TICK, count)
            for stride in (n, n + 5):
                rows = _mask_rows(rng, count, n, stride)
                if count == 3:
                    rows[0, :n], rows[1, :n], rows[2, :n] = 0, 255, 0
                    rows[2, 1] = 1
                mask = torch.from_numpy(rows).cuda()
                out = Guarded(torch, count)
                capi.check(lib.gymnet_sample_discrete_masked_device(0, None, C.c_void_p(out.ptr), count, n, start, C.c_void_p(mask.data_ptr()),
                                                                    stride, SEED, lane_offset, TICK))
                out.check(R.discrete_sample_masked(a, rows, n, start), (count, lane_offset, stride))
            shared_rows = _mask_rows(rng, 8, n, n)
            for shared in (shared_rows[1], shared_rows[0], shared_rows[3], shared_rows[5], np.ones(n, np.uint8)):
                mask = torch.from_numpy(np.ascontiguousarray(shared)).cuda()
                out = Guarded(torch, count)
                capi.check(lib.gymnet_sample_discrete_masked_device(0, None, C.c_void_p(out.ptr), count, n, start, C.c_void_p(mask.data_ptr()),
                                                                    0, SEED, lane_offset, TICK))
                out.check(R.discrete_sample_masked(a, shared, n, start), (count, lane_offset, "shared", shared.tolist()))


@pytest.mark.parametrize("name,nvals", [("CartPole-v1", 2), ("Acrobot-v1", 3)])
def test_composer_at_an_epsilon_that_equals_a_lanes_coin(api, gpu_pkg, oracle, name, nvals):
    """coin_threshold turns u <= epsilon into an integer compare: at epsilon == a lane's own coin that lane explores, at the float
    just below it keeps its policy action; the whole vector equals the reference there and at 2^-24 and 1 - 2^-24."""
    torch = api[0]
    n, off = 4099, 4102
    a, b = R.words(oracle, SEED, off, TICK, n)
    rng = np.random.default_rng(nvals)
    policy = rng.integers(0, nvals, n).astype(np.int32)
    drawn = R.discrete_sample(a, nvals, 0)
    top = b >> 8
    lane = int(np.nonzero((top > (1 << 20)) & (top < (1 << 23)))[0][0])     # a coin well inside (0, 1)
    policy[lane] = (drawn[lane] + 1) % nvals                             # exploring is visible on that lane
    eps0 = np.float32(int(top[lane]) / R.TWO24)
    below = np.nextafter(eps0, np.float32(0))
    assert float(eps0) * R.TWO24 == int(top[lane]) and below < eps0
    d_policy = torch.from_numpy(policy).cuda()
    with gpu_pkg.VectorEnv(name, n, seed=1, lane_offset=off) as env:
        for eps in (eps0, below, np.float32(2.0 ** -24), np.float32(1.0 - 2.0 ** -24)):
            out = Guarded(torch, n)
            env.ComposeActionsDevice(d_policy, float(eps), out.ptr, seed=SEED, tick=TICK); env.Sync()
            want = R.compose_discrete(a, b, nvals, eps, policy)
            out.check(want, (name, float(eps)))                          # and `out` is not written past n
            assert np.array_equal(want, oracle.compose_discrete(SEED, off, TICK, nvals, float(eps), policy))
            if eps == eps0:
                assert want[lane] == drawn[lane] != policy[lane]
            if eps == below:
                assert want[lane] == policy[lane]
    # epsilon == 0 still explores where the coin is exactly 0 (u <= 0): a committed lane with word B >> 8 == 0, and no other lane
    zero_lane = R.B_ZERO[0]
    off = zero_lane - 2049
    a, b = R.words(oracle, R.EXTREME_SEED, off, R.EXTREME_TICK, n)
    drawn = R.discrete_sample(a, nvals, 0)
    policy = ((drawn + 1) % nvals).astype(np.int32)                      # every lane's policy action differs from its draw
    d_policy = torch.from_numpy(policy).cuda()
    with gpu_pkg.VectorEnv(name, n, seed=1, lane_offset=off) as env:
        out = Guarded(torch, n)
        env.ComposeActionsDevice(d_policy, 0.0, out.ptr, seed=R.EXTREME_SEED, tick=R.EXTREME_TICK); env.Sync()
        want = policy.copy()
        want[2049] = drawn[2049]
        assert np.array_equal(want, R.compose_discrete(a, b, nvals, 0.0, policy))
        out.check(want, (name, "epsilon 0"))
