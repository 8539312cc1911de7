"""GPU checks of gymnet_gae_device / VectorEnv.AdvantagesDevice (gym.net_amd/csrc/advantage.hip).  The quantity is specified in float32,
operation for operation, so every comparison with the C twin (tests/_advantage_twin.py) is on bits; a NaN matches any NaN.  Shapes are the
smallest that can go wrong: n in {1, 3, 4, 252, 1028, 1030} (a single thread, a partial wave, a second block holding one thread, a ragged
scalar tail; the picker runs V = 1 below 2^18 lanes) x T in {1, 2, U-1, U, U+1, 2U+1, 33} around the U rows each V keeps in flight (8 and
4), each with stride = n, n + 12, n + 1 and a base offset of one element, with and without values and boot; and, since V = 4 starts at
2^18 lanes, n in {2^18, 2^18 + 4, 2^18 + 252} (whole blocks, a last block holding one thread, a partial last wave) over the same T with
every form and layout at T = 9: stride n + 12 keeps V = 4, stride n + 1 and the offset base force V = 1.  The pad columns, the elements
ahead of an offset base and the elements past the last row keep a sentinel.  Every row of tests/_advantage_forms.py is launched by name.
[T + 1, n] values against [T, n] + last_value, a NULL output, both in-place forms, a fused actor rollout followed by the call with no
synchronise in between, and refusals that write nothing.  Every test fails without the feature: the export and the method do
not exist."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _actor_twin as atwin
import _advantage_forms as forms
import _advantage_twin as twin

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = F32(-7.25)
GAMMA, LAM = 0.99, 0.95
TAIL = 8                                   # sentinel elements kept past the last row of every array


def _lib(pkg):
    capi = importlib.import_module(pkg.__name__ + "._capi")
    return capi, capi.load_library()


class Planted:
    """a host array [T, n] placed as rows of `stride` elements at element `offset` of a device buffer that is sentinel everywhere else"""

    def __init__(self, a, T, n, stride, offset, dtype):
        import torch
        self.T, self.n, self.stride, self.offset = T, n, stride, offset
        fill = SENTINEL if dtype == F32 else 0xEE
        host = np.full(offset + T * stride + TAIL, fill, dtype)
        if a is not None:
            rows = host[offset:offset + T * stride].reshape(T, stride)
            rows[:, :n] = a
        self.planted = host.copy()
        self.t = torch.from_numpy(host).cuda()
        self.ptr = self.t.data_ptr() + offset * host.itemsize

    def rows(self):
        """(the [T, n] block, True where everything outside it still holds what was planted)"""
        got = self.t.cpu().numpy()
        block = got[self.offset:self.offset + self.T * self.stride].reshape(self.T, self.stride)[:, :self.n].copy()
        rest, want = got.copy(), self.planted.copy()
        for x in (rest, want):
            x[self.offset:self.offset + self.T * self.stride].reshape(self.T, self.stride)[:, :self.n] = 0
        return block, bool(np.array_equal(rest.view(np.uint8), want.view(np.uint8)))


def _launch(pkg, c, T, n, pad=0, offset=0, values=True, boot=True, adv=True, ret=True, gamma=GAMMA, lam=LAM):
    """gymnet_gae_device on the default stream over the case's arrays in the given layout -> (advantage, return) blocks (None where not asked)"""
    import torch
    capi, lib = _lib(pkg)
    stride = n + pad
    r = Planted(c["r"], T, n, stride, offset, F32)
    d = Planted(c["d"], T, n, stride, offset, np.uint8)
    v = Planted(c["v"][:T], T, n, stride, offset, F32) if values else None
    vlast = Planted(c["v"][T:T + 1], 1, n, n, offset, F32) if values else None
    b = Planted(c["boot"], T, n, stride, offset, F32) if boot else None
    out_a = Planted(None, T, n, stride, offset, F32) if adv else None
    out_r = Planted(None, T, n, stride, offset, F32) if ret else None
    torch.cuda.synchronize()
    p = lambda x: None if x is None else C.c_void_p(x.ptr)
    capi.check(lib.gymnet_gae_device(0, None, T, n, stride, p(r), p(d), p(v), p(vlast), p(b), gamma, lam, p(out_a), p(out_r)))
    torch.cuda.synchronize()
    res = []
    for o in (out_a, out_r):
        if o is None:
            res.append(None)
            continue
        block, kept = o.rows()
        assert kept, "an element outside [T][n] was written"
        res.append(block)
    for x in (r, d, v, vlast, b):                                 # the inputs are read only
        if x is not None:
            assert np.array_equal(x.t.cpu().numpy().view(np.uint8), x.planted.view(np.uint8))
    return res


def _want(c, T, values=True, boot=True, gamma=GAMMA, lam=LAM):
    return twin.gae(c["r"], c["d"], c["v"][:T] if values else None, c["v"][T] if values else None, c["boot"] if boot else None, gamma, lam)


LAYOUTS = ((0, 0), (12, 0), (1, 0), (0, 1))                       # (stride - n, base offset in elements)
STEPS = twin.steps_for(forms.U.values())
FORM_SET = ((True, True), (True, False), (False, True), (False, False))      # (values, boot)


@pytest.mark.parametrize("n", twin.NS)
def test_every_shape_layout_and_form_has_the_twins_bits(gpu_pkg, n):
    reached = set()
    for T in STEPS:
        c = twin.case(T, n)
        if T == 33:
            c["r"][T // 2, 0] = np.nan                            # a NaN input: NaN where the twin has NaN
        for values, boot in FORM_SET:
            want = _want(c, T, values, boot)
            for pad, offset in LAYOUTS:
                got = _launch(gpu_pkg, c, T, n, pad, offset, values, boot)
                assert twin.same(got[0], want[0]) and twin.same(got[1], want[1]), (T, n, pad, offset, values, boot)
                reached.add(forms.kernel_for(n, n + pad, offset % 4 == 0, values, boot))
    assert reached == {row["kernel"] for row in forms.FORMS if row["vec"] == 1}     # fewer than 2^18 lanes: V = 1


@pytest.mark.parametrize("n", twin.WIDE_NS)
def test_the_lane_counts_where_four_lanes_per_thread_run(gpu_pkg, n):
    """V = 4 starts at 2^18 lanes: every T with values and boot, and at T = 9 every form in every layout (V = 4 and, forced, V = 1)"""
    reached = set()
    for T in STEPS:
        c = twin.case(T, n)
        if T == 33:
            c["r"][T // 2, 5] = np.nan
        for values, boot in (FORM_SET if T == twin.WIDE_T else FORM_SET[:1]):
            want = _want(c, T, values, boot)
            for pad, offset in (LAYOUTS if T == twin.WIDE_T else LAYOUTS[:1]):
                got = _launch(gpu_pkg, c, T, n, pad, offset, values, boot)
                assert twin.same(got[0], want[0]) and twin.same(got[1], want[1]), (T, n, pad, offset, values, boot)
                reached.add(forms.kernel_for(n, n + pad, offset % 4 == 0, values, boot))
    assert reached == {row["kernel"] for row in forms.FORMS}


@pytest.mark.parametrize("row", forms.FORMS, ids=lambda row: row["kernel"])
def test_every_row_of_the_forms_table_is_launched(gpu_pkg, row):
    reach = row["reach"]
    n, T = reach["count"], 2 * forms.U[row["vec"]] + 1
    assert forms.kernel_for(n, n + reach["pad"], reach["offset"] % 4 == 0, row["values"], row["boot"]) == row["kernel"]
    c = twin.case(T, n, seed=2)
    got = _launch(gpu_pkg, c, T, n, reach["pad"], reach["offset"], row["values"], row["boot"])
    want = _want(c, T, row["values"], row["boot"])
    assert twin.same(got[0], want[0]) and twin.same(got[1], want[1])


@pytest.mark.parametrize("n", [1030, twin.WIDE_NS[1]])
def test_a_null_output_leaves_the_others_bits_unchanged(gpu_pkg, n):
    T = 9
    c = twin.case(T, n, seed=3)
    want = _want(c, T)
    only_adv = _launch(gpu_pkg, c, T, n, ret=False)
    only_ret = _launch(gpu_pkg, c, T, n, adv=False)
    assert only_adv[1] is None and only_ret[0] is None
    assert twin.same(only_adv[0], want[0]) and twin.same(only_ret[1], want[1])


@pytest.mark.parametrize("n", [252, twin.WIDE_NS[0]])
def test_special_settings_have_the_twins_bits(gpu_pkg, n):
    T = 33 if n < forms.NARROW_BELOW else twin.WIDE_T
    c = twin.case(T, n, seed=4)
    for gamma, lam in ((0.99, 0.0), (0.0, 0.95), (1.0, 1.0), (0.0, 0.0)):
        for values in (True, False):
            got = _launch(gpu_pkg, c, T, n, values=values, gamma=gamma, lam=lam)
            want = _want(c, T, values, True, gamma, lam)
            assert twin.same(got[0], want[0]) and twin.same(got[1], want[1]), (gamma, lam, values)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("n", [1030, twin.WIDE_NS[0]])
def test_the_python_surface_values_layouts_and_in_place_forms(gpu_pkg, n):
    """through VectorEnv.AdvantagesDevice on a handle's stream: [T + 1, n] values against [T, n] + last_value, the lean form, and both
    in-place forms against the out-of-place bits"""
    import torch
    T = 2 * forms.U[4 if n >= forms.NARROW_BELOW else 1] + 1
    c = twin.case(T, n, seed=5)
    want = _want(c, T)
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=1) as env:
        def run(values, last_value, adv, ret, boot=c["boot"], reward=None):
            torch.cuda.synchronize()                               # the uploads (torch's stream) end before the handle's stream reads
            env.AdvantagesDevice(_t(c["r"]) if reward is None else reward, _t(c["d"]), values, adv, ret, GAMMA, LAM, last_value=last_value,
                                 boot=None if boot is None else _t(boot))
            env.Sync()
        new = lambda: torch.full((T, n), float(SENTINEL), dtype=torch.float32, device="cuda")
        a1, r1 = new(), new()
        run(_t(c["v"][:T]), _t(c["v"][T]), a1, r1)
        a2, r2 = new(), new()
        run(_t(c["v"]), None, a2, r2)
        for a, r in ((a1, r1), (a2, r2)):
            assert twin.same(a.cpu().numpy(), want[0]) and twin.same(r.cpu().numpy(), want[1])
        a3 = new()
        run(None, None, a3, None, boot=None)
        assert twin.same(a3.cpu().numpy(), twin.gae(c["r"], c["d"], None, None, None, GAMMA, LAM)[0])
        # in place: advantage over reward and return over value ...
        rew, val = _t(c["r"]), _t(c["v"][:T])
        run(val, _t(c["v"][T]), rew, val, reward=rew)
        assert twin.same(rew.cpu().numpy(), want[0]) and twin.same(val.cpu().numpy(), want[1])
        # ... and advantage over value, return over reward
        rew, val = _t(c["r"]), _t(c["v"][:T])
        run(val, _t(c["v"][T]), val, rew, reward=rew)
        assert twin.same(val.cpu().numpy(), want[0]) and twin.same(rew.cpu().numpy(), want[1])
        # ... and over the first T rows of a [T + 1, n] values tensor, whose row T stays
        rew, val = _t(c["r"]), _t(c["v"])
        run(val, None, rew, val, reward=rew)
        got = val.cpu().numpy()
        assert twin.same(rew.cpu().numpy(), want[0]) and twin.same(got[:T], want[1]) and twin.same(got[T], c["v"][T])


def test_after_a_fused_actor_rollout_with_no_synchronise_in_between(gpu_pkg):
    """CartPole, 260 lanes, T = 8 with a time limit of 5 steps so that both done bits occur: the rollout records reward and done, the call
    follows on the same stream at once, and the result equals the twin over the recorded arrays read back afterwards"""
    import torch
    n, T = 260, 8
    rng = np.random.default_rng(9)
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=3, auto_reset=True, episode_stats=True, max_episode_steps=5) as env:
        env.Reset()
        _, _, pairs = atwin.net(rng, [16, 50, 20, 2])
        env.Actor(pairs, 4)
        rec_reward = torch.zeros((T, n), dtype=torch.float32, device="cuda")
        rec_done = torch.zeros((T, n), dtype=torch.uint8, device="cuda")
        values = _t(rng.standard_normal((T + 1, n)).astype(F32))
        boot = _t(rng.standard_normal((T, n)).astype(F32))
        adv = torch.full((T, n), float(SENTINEL), dtype=torch.float32, device="cuda")
        ret = torch.full((T, n), float(SENTINEL), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        env.RolloutFusedDevice(None, T, actions="actor", epsilon=0.3, action_seed=5, action_tick0=0, rec_reward=rec_reward, rec_done=rec_done)
        env.AdvantagesDevice(rec_reward, rec_done, values, adv, ret, GAMMA, LAM, boot=boot)
        env.Sync()
        r, d, v, b = rec_reward.cpu().numpy(), rec_done.cpu().numpy(), values.cpu().numpy(), boot.cpu().numpy()
        assert (d & 2).any() and (r != 0).any()                     # the rollout did record, and a time limit did truncate
        want = twin.gae(r, d, v[:T], v[T], b, GAMMA, LAM)
        assert twin.same(adv.cpu().numpy(), want[0]) and twin.same(ret.cpu().numpy(), want[1])


def test_refusals_name_their_reason_and_write_nothing(gpu_pkg):
    import torch
    capi, lib = _lib(gpu_pkg)
    T, n = 5, 252
    c = twin.case(T, n, seed=6)
    r, d, v, vlast, b = _t(c["r"]), _t(c["d"]), _t(c["v"][:T]), _t(c["v"][T]), _t(c["boot"])
    adv = torch.full((T, n), float(SENTINEL), dtype=torch.float32, device="cuda")
    ret = torch.full((T, n), float(SENTINEL), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    good = dict(steps=T, count=n, stride=n, r=r, d=d, v=v, vlast=vlast, b=b, gamma=GAMMA, lam=LAM, adv=adv, ret=ret)

    def call(**change):
        a = dict(good, **change)
        return lib.gymnet_gae_device(0, None, a["steps"], a["count"], a["stride"], p(a["r"]), p(a["d"]), p(a["v"]), p(a["vlast"]), p(a["b"]),
                                     a["gamma"], a["lam"], p(a["adv"]), p(a["ret"]))
    refused = [dict(gamma=1.5), dict(gamma=-0.5), dict(gamma=float("nan")), dict(lam=1.5), dict(lam=float("inf")), dict(stride=n - 1),
               dict(steps=-1), dict(count=-1), dict(adv=None, ret=None), dict(ret=adv), dict(adv=b), dict(ret=vlast), dict(r=None), dict(d=None)]
    for change in refused:
        assert call(**change) == capi.ERR_INVALID_ARG, change
        assert lib.gymnet_last_error().decode().startswith("gae:"), change
    torch.cuda.synchronize()
    for x, was in ((adv, None), (ret, None), (r, c["r"]), (v, c["v"][:T]), (b, c["boot"]), (vlast, c["v"][T])):
        got = x.cpu().numpy()
        assert (got == SENTINEL).all() if was is None else twin.same(got, was)
    assert call(steps=0) == 0 and call(count=0, stride=0) == 0     # a successful no-op
    torch.cuda.synchronize()
    assert (adv.cpu().numpy() == SENTINEL).all() and (ret.cpu().numpy() == SENTINEL).all()
    assert call() == 0                                             # and the good call computes
    torch.cuda.synchronize()
    want = _want(c, T)
    assert twin.same(adv.cpu().numpy(), want[0]) and twin.same(ret.cpu().numpy(), want[1])
