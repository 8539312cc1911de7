"""GPU checks of gymnet_rollout_inputs_device / VectorEnv.RolloutInputsDevice (gym.net_amd/csrc/rollout_inputs.hip) and of
gymnet_vecenv_actor_history_device / Actor.HistoryDevice.  The call is data movement specified bit for bit, so every output is compared as
uint32 bit patterns with the NumPy twin (tests/_rollout_inputs_twin.py), NaN payloads included.  Every buffer is planted in a larger one
that holds a sentinel: the pad columns, the floats between output rows, a guard band ahead of the first row and past the last one must
keep it.  Shapes are the smallest that can go wrong: (obs_dim, S) from one slot to the widest input an actor can have, widths that are
and are not a multiple of 4; 1, 3, 67, 256, 1028 lanes (a single thread, a partial wave, a ragged block, whole blocks, a second block's
tail) with stride = count and count + 5; T in {1, 2, S-1, S, S+1, 37} around the look-back of S - 1 rows, the rows kept in flight (4) and
the chunk floor (8 rows, or S); x_row_stride = the width and the width + 3 (which forces one float per thread).  Every test fails without
the feature: the exports and the methods do not exist."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _actor_logp_twin as ltwin
import _actor_twin as atwin
import _rollout_inputs_forms as forms
import _rollout_inputs_twin as twin

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32
FRONT, TAIL = 16, 16                       # sentinel elements kept ahead of every array and past it
SENTINEL = {np.dtype(U32): 0xDEADBEEF, np.dtype(np.uint8): 0xEE, np.dtype(np.float64): -7.25, np.dtype(np.int64): -99}


def _lib(pkg):
    capi = importlib.import_module(pkg.__name__ + "._capi")
    return capi, capi.load_library()


class Planted:
    """a host array [rows, n] placed as rows of `stride` elements, `offset` elements past the front guard of a device buffer that holds
    the sentinel everywhere else; a is None: an output"""

    def __init__(self, a, rows, n, stride, dtype, offset=0):
        import torch
        dtype = np.dtype(dtype)
        self.rows_, self.n, self.stride, self.first = rows, n, stride, FRONT + offset
        host = np.full(self.first + rows * stride + TAIL, SENTINEL[dtype], dtype)
        if a is not None:
            self._block(host)[...] = np.asarray(a).reshape(rows, n)
        self.planted = host.copy()
        self.t = torch.from_numpy(host.view(np.int32) if dtype == U32 else host).cuda()
        self.dtype = dtype
        self.ptr = self.t.data_ptr() + self.first * dtype.itemsize

    def _block(self, host):
        return host[self.first:self.first + self.rows_ * self.stride].reshape(self.rows_, self.stride)[:, :self.n]

    def read(self):
        """(the [rows, n] block, True where everything outside it still holds what was planted)"""
        got = self.t.cpu().numpy().view(self.dtype)
        block = self._block(got).copy()
        rest, want = got.copy(), self.planted.copy()
        self._block(rest)[...] = 0
        self._block(want)[...] = 0
        return block, bool(np.array_equal(rest.view(np.uint8), want.view(np.uint8)))

    def unchanged(self):
        return bool(np.array_equal(self.t.cpu().numpy().view(np.uint8), self.planted.view(np.uint8)))


def _launch(pkg, c, pad=0, x_pad=0, rows=None, history_out=True, x_off=0, obs_off=0, steps=None, row0=0, history0=None):
    """gymnet_rollout_inputs_device on the default stream over a case's arrays in the given layout -> (x uint32 [rows, W], history_out
    uint32 [S, O, n] or None, the names of the kernels the mirror says ran).  steps / row0 / history0: a part of the case's rows."""
    import torch
    capi, lib = _lib(pkg)
    S, O, n = c["history0"].shape
    T = c["rec_obs"].shape[0] - row0 if steps is None else steps
    W, stride = S * O, n + pad
    f64 = c["rec_obs"].dtype == np.float64
    obs_bits = c["rec_obs"][row0:row0 + T] if f64 else c["rec_obs"][row0:row0 + T].view(U32)
    obs = Planted(obs_bits, T * O, n, stride, np.float64 if f64 else U32, obs_off)
    done = Planted(c["rec_done"][row0:row0 + T], T, n, stride, np.uint8, 1)                 # (an odd address: any byte serves)
    h0 = Planted((c["history0"] if history0 is None else history0).view(U32), W, n, stride, U32)
    idx = None if rows is None else Planted(np.asarray(rows, np.int64), 1, len(rows), len(rows), np.int64)
    m = T * n if rows is None else len(rows)
    x = Planted(None, m, W, W + x_pad, U32, x_off)
    hout = Planted(None, W, n, n + 2 * pad, U32) if history_out else None
    torch.cuda.synchronize()
    p = lambda v: None if v is None else C.c_void_p(v.ptr)
    capi.check(lib.gymnet_rollout_inputs_device(0, None, T, n, stride, O, S, 1 if f64 else 0, p(obs), p(done), p(h0), stride, p(idx), 0 if idx is None else m,
                                                p(x), W + x_pad, p(hout), n + 2 * pad))
    torch.cuda.synchronize()
    got_x, kept = x.read()
    assert kept, "an element outside the output rows was written"
    got_h = None
    if hout is not None:
        got_h, kept = hout.read()
        assert kept, "an element outside d_history_out's columns was written"
        got_h = got_h.reshape(S, O, n)
    for inp in (obs, done, h0, idx):                                # the inputs are read only
        assert inp is None or inp.unchanged()
    return got_x, got_h, forms.kernels_for(O, S, W + x_pad, x.ptr, f64, rows is not None, history_out)


def _dense(pkg, c, **kw):
    x, h, ran = _launch(pkg, c, **kw)
    return x.reshape(c["x"].shape[0] if "steps" not in kw else kw["steps"], -1, x.shape[-1]), h, ran


LAYOUTS = ((0, 0), (5, 3), (0, 3), (5, 0))                         # (stride - count, x_row_stride - width)


@pytest.mark.parametrize("O,S", twin.SHAPES)
def test_dense_rows_and_the_last_history_have_the_twins_bits(gpu_pkg, O, S):
    ran, k = set(), 0
    cases = [(n, T, twin.PATTERNS[(i + j) % len(twin.PATTERNS)]) for i, n in enumerate(twin.COUNTS) for j, T in enumerate(twin.steps_for(S))]
    cases += [(67, 37, pattern) for pattern in twin.PATTERNS]     # every done pattern at one shape, in both extreme layouts
    for n, T, pattern in cases:
        c = twin.case(O, S, T, n, pattern)
        layouts = LAYOUTS[:2] + (LAYOUTS[2 + k % 2],)               # both strides and both row strides each time, the crossed pairs in turn
        k += 1
        for pad, x_pad in layouts:
            x, h, names = _dense(gpu_pkg, c, pad=pad, x_pad=x_pad)
            assert np.array_equal(x, c["x"]), (n, T, pattern, pad, x_pad, np.argwhere(x != c["x"])[:4])
            assert np.array_equal(h, c["history_out"]), (n, T, pattern, pad, x_pad)
            ran |= names
    want = {forms.row_kernel(1, False, False), forms.history_kernel(False)}
    if (O * S) % 4 == 0:
        want.add(forms.row_kernel(4, False, False))
    assert ran == want


@pytest.mark.parametrize("O,S", [(4, 4), (3, 21), (1, 64)])
def test_float64_observations_are_rounded_once_to_nearest_even(gpu_pkg, O, S):
    for n in (3, 67, 1028):
        for T in (2, S + 1, 37):
            c = twin.case(O, S, T, n, "bernoulli", f64=True)
            assert T * O * n < len(twin.F64_SPECIALS) or np.isinf(twin.f32_bits(c["rec_obs"]).view(F32)).any()       # the planted values are in
            for pad, x_pad in LAYOUTS[:2]:
                x, h, _ = _dense(gpu_pkg, c, pad=pad, x_pad=x_pad)
                bad = np.argwhere(x != c["x"])[:4]
                assert np.array_equal(x, c["x"]), (n, T, pad, x_pad, bad, [hex(v) for v in x[tuple(bad.T)]], [hex(v) for v in c["x"][tuple(bad.T)]])
                assert np.array_equal(h, c["history_out"]), (n, T, pad, x_pad)
            rows = np.random.default_rng(T).integers(0, T * n, 2 * n + 1)
            gx, gh, _ = _launch(gpu_pkg, c, rows=rows)
            assert np.array_equal(gx, twin.gathered(c["x"], rows)) and np.array_equal(gh, c["history_out"])


@pytest.mark.parametrize("O,S", twin.SHAPES)
def test_gathered_rows_equal_the_dense_rows_they_name(gpu_pkg, O, S):
    ran = set()
    for n in (1, 67, 1028):
        for T in (1, S + 1, 37):
            c = twin.case(O, S, T, n, "runs" if T > 1 else "first_row")
            rng = np.random.default_rng([n, T])
            many = rng.integers(0, T * n, T * n + 9)                # more rows than steps * count: duplicates are certain
            many[:2] = (T * n - 1, 0)
            for rows, pad, x_pad in ((many, 0, 0), (many[:min(300, len(many))], 5, 3), (many[:1], 0, 0), (many[3:4], 5, 3)):
                x, h, names = _launch(gpu_pkg, c, rows=rows, pad=pad, x_pad=x_pad)
                assert np.array_equal(x, twin.gathered(c["x"], rows)), (n, T, len(rows), pad, x_pad)
                assert np.array_equal(h, c["history_out"])
                ran |= names
            # indices outside [0, T * n): a row of canonical NaNs each, the neighbours intact, nothing else written (Planted's guard)
            rows = many[:9].copy()
            rows[4] = T * n
            x, _, _ = _launch(gpu_pkg, c, rows=rows, history_out=False)
            assert (x[4] == twin.NAN_BITS).all() and np.array_equal(x, twin.gathered(c["x"], rows))
            rows[[0, 8]] = (-1, 2 ** 40)
            x, _, _ = _launch(gpu_pkg, c, rows=rows, x_pad=3, history_out=False)
            assert (x[[0, 4, 8]] == twin.NAN_BITS).all() and np.array_equal(x, twin.gathered(c["x"], rows))
    want = {forms.row_kernel(1, False, True), forms.history_kernel(False)}
    if (O * S) % 4 == 0:
        want.add(forms.row_kernel(4, False, True))
    assert ran == want


@pytest.mark.parametrize("O,S", twin.SHAPES)
def test_a_rollout_cut_in_two_chains_through_the_history(gpu_pkg, O, S):
    T = max(37, S + 5)                                              # (T1 = S - 1 needs S - 1 < T)
    for n, pattern in ((3, "runs"), (1028, "bernoulli")):
        c = twin.case(O, S, T, n, pattern)
        for T1 in sorted({1, max(S - 1, 1), T - 1}):
            xa, ha, _ = _dense(gpu_pkg, c, steps=T1)
            xb, hb, _ = _dense(gpu_pkg, c, steps=T - T1, row0=T1, history0=ha.view(F32), pad=5, x_pad=3)
            assert np.array_equal(np.concatenate([xa, xb]), c["x"]), (n, T1)
            assert np.array_equal(hb, c["history_out"]), (n, T1)


def test_no_steps_or_no_rows(gpu_pkg):
    """steps == 0 writes only d_history_out = H_0, in either form; the gathered form with no row writes nothing at all"""
    capi, lib = _lib(gpu_pkg)
    c = twin.case(4, 4, 2, 67, "none")
    for rows in (None, [0, 1, 2]):
        x, h, _ = _launch(gpu_pkg, c, steps=0, rows=rows, pad=5)
        assert np.array_equal(h, c["history0"].view(U32))
        assert rows is None or (x == SENTINEL[np.dtype(U32)]).all()            # no row was written (Planted checked the rest)
    import torch
    obs, done, h0 = (torch.from_numpy(np.array(c[k])).cuda() for k in ("rec_obs", "rec_done", "history0"))
    x = torch.full((8, 16), -7.25, dtype=torch.float32, device="cuda")
    hout = torch.full((4, 4, 67), -7.25, dtype=torch.float32, device="cuda")
    rows = torch.zeros(8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())
    capi.check(lib.gymnet_rollout_inputs_device(0, None, 2, 67, 67, 4, 4, 0, p(obs), p(done), p(h0), 67, p(rows), 0, p(x), 16, p(hout), 67))
    torch.cuda.synchronize()
    assert (x.cpu().numpy() == -7.25).all() and (hout.cpu().numpy() == -7.25).all()


@pytest.mark.parametrize("row", forms.FORMS, ids=lambda row: row["kernel"])
def test_every_row_of_the_forms_table_is_launched(gpu_pkg, row):
    """No lane-count threshold selects four floats per thread, so the smallest count that reaches it is 1: each row runs at 1 and at 1028
    lanes with T = 6.  At 1028 lanes a d_x off its 16-byte boundary falls back to one float per thread, a d_rec_obs off its 16-byte
    boundary changes nothing, and both give the same bits."""
    r = row["reach"]
    O, S, T = r["obs_dim"], r["history"], 6
    for n in (1, 1028):
        c = twin.case(O, S, T, n, "bernoulli", seed=2, f64=row["f64"])
        rows = np.random.default_rng(n).integers(0, T * n, 3 * n) if row["gathered"] else None
        want = c["x"].reshape(-1, O * S) if rows is None else twin.gathered(c["x"], rows)
        x, h, ran = _launch(gpu_pkg, c, rows=rows, x_pad=r["pad"], x_off=r["offset"])
        assert ran == {row["kernel"], forms.history_kernel(row["f64"])}
        assert np.array_equal(x, want) and np.array_equal(h, c["history_out"])
    fallback = forms.row_kernel(1, row["f64"], row["gathered"])
    for x_off in (1, 2, 3):
        x, h, ran = _launch(gpu_pkg, c, rows=rows, x_pad=r["pad"], x_off=x_off)
        assert fallback in ran and np.array_equal(x, want) and np.array_equal(h, c["history_out"])
    x, h, ran = _launch(gpu_pkg, c, rows=rows, x_pad=r["pad"], obs_off=1)
    assert row["kernel"] in ran and np.array_equal(x, want) and np.array_equal(h, c["history_out"])


def test_more_than_one_chunk_of_rows(gpu_pkg):
    """the picker cuts 37 steps of 67 lanes into five chunks of 8 rows and 100 steps at S = 32 into four of 32: each chunk's first row looks
    back into the chunk before it, or into d_history0"""
    assert forms.chunks_for(37, 67, 4, 4, 4) == (8, 5) and forms.chunks_for(100, 67, 2, 32, 4) == (32, 4)
    for O, S, T in ((4, 4, 37), (2, 32, 100), (3, 21, 100)):
        for pattern in ("none", "runs", "bernoulli"):
            c = twin.case(O, S, T, 67, pattern, seed=3)
            x, h, _ = _dense(gpu_pkg, c)
            assert np.array_equal(x, c["x"]) and np.array_equal(h, c["history_out"]), (O, S, pattern)


def test_refusals_name_their_reason_and_write_nothing(gpu_pkg):
    import torch
    capi, lib = _lib(gpu_pkg)
    O, S, T, n = 4, 4, 5, 67
    c = twin.case(O, S, T, n, "bernoulli", seed=4)
    t = lambda a: torch.from_numpy(np.array(a)).cuda()
    obs, done, h0 = t(c["rec_obs"]), t(c["rec_done"]), t(c["history0"])
    rows = t(np.arange(7, dtype=np.int64))
    x = torch.full((T * n * S * O + 8,), -7.25, dtype=torch.float32, device="cuda")
    hout = torch.full((S * O * n + 8,), -7.25, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    good = dict(steps=T, count=n, stride=n, obs_dim=O, history=S, f64=0, obs=obs.data_ptr(), done=done.data_ptr(), h0=h0.data_ptr(), h0s=n, rows=None, m=0,
                x=x.data_ptr(), xrs=S * O, hout=hout.data_ptr(), hs=n)

    def call(**change):
        a = dict(good, **change)
        p = lambda v: None if v is None else C.c_void_p(v)
        return lib.gymnet_rollout_inputs_device(0, None, a["steps"], a["count"], a["stride"], a["obs_dim"], a["history"], a["f64"], p(a["obs"]), p(a["done"]),
                                                p(a["h0"]), a["h0s"], p(a["rows"]), a["m"], p(a["x"]), a["xrs"], p(a["hout"]), a["hs"])
    refused = [dict(steps=-1), dict(count=-1), dict(stride=n - 1), dict(h0s=n - 1), dict(hs=n - 1), dict(xrs=S * O - 1), dict(xrs=-1), dict(obs_dim=0), dict(history=0),
               dict(history=17), dict(obs=None), dict(done=None), dict(h0=None), dict(x=None), dict(rows=rows.data_ptr(), m=7, x=None), dict(rows=rows.data_ptr(), m=-1),
               dict(obs=good["obs"] + 2), dict(f64=1, obs=good["obs"] + 4), dict(h0=good["h0"] + 1), dict(x=good["x"] + 2), dict(hout=good["hout"] + 3),
               dict(rows=rows.data_ptr() + 4, m=6), dict(x=good["obs"]), dict(x=good["h0"]), dict(hout=good["h0"]), dict(hout=good["obs"]), dict(hout=good["x"]),
               dict(rows=rows.data_ptr(), m=7, x=rows.data_ptr())]
    for change in refused:
        assert call(**change) == capi.ERR_INVALID_ARG, change
        assert lib.gymnet_last_error().decode().startswith("rollout_inputs: "), change
    torch.cuda.synchronize()
    assert (x.cpu().numpy() == -7.25).all() and (hout.cpu().numpy() == -7.25).all()
    for inp, was in ((obs, c["rec_obs"]), (h0, c["history0"])):
        assert np.array_equal(inp.cpu().numpy().view(U32), was.view(U32))
    assert np.array_equal(done.cpu().numpy(), c["rec_done"]) and np.array_equal(rows.cpu().numpy(), np.arange(7))
    assert call() == 0                                             # and the good call computes
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy().view(U32)[:T * n * S * O].reshape(T, n, S * O), c["x"])
    assert np.array_equal(hout.cpu().numpy().view(U32)[:S * O * n].reshape(S, O, n), c["history_out"])


# ---- end to end: a fused actor rollout's inputs ----------------------------------------------------------------------------------------
ENVS = {"CartPole-v1": [16, 20, 2], "Acrobot-v1": [24, 16, 3], "Pendulum-v1": [12, 16, 1]}
S_E2E, T_E2E, WARM = 4, 48, 3


def _bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


@pytest.mark.parametrize("n", [67, 256])
@pytest.mark.parametrize("name", list(ENVS))
def test_the_inputs_of_a_fused_actor_rollout_are_what_single_steps_read(gpu_pkg, name, n):
    """Two handles from the same seeds, auto-reset with a time limit of 20 steps so that both done bits occur within T = 48, a few
    closed-loop steps first (a mid-episode start).  Handle a: h0 = HistoryDevice(), one fused actor rollout, RolloutInputsDevice with no
    synchronise in between.  Handle b: T x actor.Step, the history read before each.  Row by row the dense x is b's history; history_out
    is the history after the rollout on both.  On CartPole under ("softmax", 1.0) at epsilon = 1 the logp twin over x[t] gives rec_logp[t]
    bit for bit: logp_old is reproducible from what the caller is handed."""
    import torch
    eps, aseed, tick0 = (1.0, 31, 500) if name == "CartPole-v1" else (0.3, 31, 500)
    rng = np.random.default_rng(17)
    w, flat, pairs = atwin.net(rng, ENVS[name])
    kw = dict(seed=5, auto_reset=True, episode_stats=True, max_episode_steps=20)
    with gpu_pkg.VectorEnv(name, n, **kw) as a, gpu_pkg.VectorEnv(name, n, **kw) as b:
        a.Reset(); b.Reset()
        O, T, S = a.ObsDim, T_E2E, S_E2E
        actor_a, actor_b = a.Actor(pairs, S), b.Actor(pairs, S)
        logp = name == "CartPole-v1"
        if logp:
            actor_a.SetExploration("softmax", 1.0); actor_b.SetExploration("softmax", 1.0)
        for t in range(WARM):
            actor_a.Step(eps, aseed + 1, t); actor_b.Step(eps, aseed + 1, t)
        h0 = actor_a.HistoryDevice()
        assert tuple(h0.shape) == (S, O, n) and np.array_equal(_bits(h0.cpu().numpy()), _bits(actor_a.History().transpose(1, 2, 0)))      # 1.
        rec = dict(rec_obs=torch.empty((T, O, n), dtype=torch.float32, device="cuda"), rec_done=torch.empty((T, n), dtype=torch.uint8, device="cuda"))
        if logp:
            rec["rec_actions"] = torch.empty((T, n), dtype=torch.int32, device="cuda")
            rec["rec_logp"] = torch.empty((T, n), dtype=torch.float32, device="cuda")
        hout = torch.full((S, O, n), -7.25, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        a.RolloutFusedDevice(None, T, actions="actor", epsilon=eps, action_seed=aseed, action_tick0=tick0, **rec)                          # 2.
        x = a.RolloutInputsDevice(rec["rec_obs"], rec["rec_done"], h0, history=S, history_out=hout)
        idx = torch.from_numpy(np.random.default_rng(3).integers(0, T * n, 500)).cuda()
        xg = a.RolloutInputsDevice(rec["rec_obs"], rec["rec_done"], h0, history=S, rows=idx)
        a.Sync()
        x = x.cpu().numpy()
        assert x.shape == (T, n, S * O)
        done = rec["rec_done"].cpu().numpy()
        assert (done & 2).any() and (name != "CartPole-v1" or (done & 1).any())      # a time limit everywhere; CartPole also falls
        for t in range(T):                                                                                                                 # 3.
            assert np.array_equal(_bits(actor_b.History().reshape(n, S * O)), _bits(x[t])), t
            actor_b.Step(eps, aseed, tick0 + t)
        assert np.array_equal(_bits(actor_b.History()), _bits(hout.cpu().numpy().transpose(2, 0, 1)))
        assert np.array_equal(_bits(actor_a.History()), _bits(actor_b.History()))
        assert np.array_equal(_bits(xg.cpu().numpy()), _bits(x.reshape(T * n, -1)[idx.cpu().numpy()]))
        # the twin over the recorded arrays agrees too
        want, want_h = twin.inputs(rec["rec_obs"].cpu().numpy(), done, h0.cpu().numpy())
        assert np.array_equal(_bits(x), want) and np.array_equal(_bits(hout.cpu().numpy()), want_h)
        if logp:                                                                                                                           # 4.
            got_logp, acts = rec["rec_logp"].cpu().numpy().view(U32), rec["rec_actions"].cpu().numpy()
            for t in range(T):
                logits, _ = atwin.forward(w, flat, x[t])
                assert np.array_equal(ltwin.logp(logits, acts[t], 1.0), got_logp[t]), t
            assert len(np.unique(acts)) == 2


def test_a_float64_handles_records_reproduce_step_and_push(gpu_pkg):
    """5.  A float64 CartPole handle: the ring rollout's float64 rec_obs with obs_f64 gives the histories of T x (StepDevice, actor.Push)"""
    import torch
    n, T, S = 67, T_E2E, S_E2E
    rng = np.random.default_rng(19)
    _, _, pairs = atwin.net(rng, ENVS["CartPole-v1"])
    actions = torch.from_numpy(rng.integers(0, 2, (T, n)).astype(np.int32)).cuda()
    kw = dict(seed=6, auto_reset=True, episode_stats=True, max_episode_steps=20, dtype=np.float64)
    with gpu_pkg.VectorEnv("CartPole-v1", n, **kw) as a, gpu_pkg.VectorEnv("CartPole-v1", n, **kw) as b:
        a.Reset(); b.Reset()
        actor_a, actor_b = a.Actor(pairs, S), b.Actor(pairs, S)
        h0 = actor_a.HistoryDevice()
        assert np.array_equal(_bits(h0.cpu().numpy()), _bits(actor_a.History().transpose(1, 2, 0)))
        rec_obs = torch.empty((T, 4, n), dtype=torch.float64, device="cuda")
        rec_done = torch.empty((T, n), dtype=torch.uint8, device="cuda")
        hout = torch.empty((S, 4, n), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        a.RolloutFusedDevice(actions, T, n, T, rec_obs=rec_obs, rec_done=rec_done)
        x = a.RolloutInputsDevice(rec_obs, rec_done, h0, history=S, history_out=hout)
        a.Sync()
        x = x.cpu().numpy()
        assert rec_done.cpu().numpy().any()
        for t in range(T):
            assert np.array_equal(_bits(actor_b.History().reshape(n, -1)), _bits(x[t])), t
            step = actions[t].clone()                                # (a float64 handle wants its actions 8-byte aligned: a row of 67 is not)
            b.StepDevice(step)
            actor_b.Push()
        assert np.array_equal(_bits(actor_b.History()), _bits(hout.cpu().numpy().transpose(2, 0, 1)))


# ---- gymnet_vecenv_actor_history_device -----------------------------------------------------------------------------------------------
def test_history_device_pad_columns_and_refusals(gpu_pkg):
    import torch
    capi, lib = _lib(gpu_pkg)
    n, S = 67, 4
    _, _, pairs = atwin.net(np.random.default_rng(23), ENVS["Pendulum-v1"])
    with gpu_pkg.VectorEnv("Pendulum-v1", n, seed=7, auto_reset=True) as env:
        env.Reset()
        O = env.ObsDim
        out = torch.full((S * O * (n + 5) + 4,), -7.25, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        call = lambda ptr, stride: lib.gymnet_vecenv_actor_history_device(env._h, None if ptr is None else C.c_void_p(ptr), stride)
        assert call(out.data_ptr(), n + 5) == capi.ERR_INVALID_ARG                                    # no actor configured
        actor = env.Actor(pairs, S)
        for t in range(6):                                                                            # the ring has wrapped
            actor.Step(0.5, 3, t)
        assert call(out.data_ptr(), n + 5) == 0                                                       # a Box actor is served
        env.Sync()
        got = out.cpu().numpy()
        block = got[:S * O * (n + 5)].reshape(S, O, n + 5)
        assert np.array_equal(_bits(block[:, :, :n]), _bits(actor.History().transpose(1, 2, 0)))
        assert (block[:, :, n:] == -7.25).all() and (got[S * O * (n + 5):] == -7.25).all()            # the pad columns are not touched
        out.fill_(-7.25)
        torch.cuda.synchronize()
        for ptr, stride in ((None, n), (out.data_ptr() + 2, n), (out.data_ptr(), n - 1), (out.data_ptr(), -1)):
            assert call(ptr, stride) == capi.ERR_INVALID_ARG, (ptr, stride)
        tick = env.Tick
        env.StepDevice(actor.Act(0.0))                                                                # a bare step: the history is stale
        assert call(out.data_ptr(), n) == capi.ERR_INVALID_ARG and "stale" in lib.gymnet_last_error().decode()
        with pytest.raises(Exception):
            actor.HistoryDevice()
        actor.Push()                                                                                  # ... and current again: no mark was moved
        assert env.Tick == tick + 1
        env.Sync()
        assert (out.cpu().numpy() == -7.25).all()                                                     # nothing was written by a refusal
        h = actor.HistoryDevice()
        mine = torch.empty((S, O, n), dtype=torch.float32, device="cuda")
        assert actor.HistoryDevice(mine) is mine
        actor.Step(0.0, 3, 9)                                                                         # the snapshot is the caller's: a later push leaves it
        env.Sync()
        assert np.array_equal(_bits(h.cpu().numpy()), _bits(mine.cpu().numpy()))
        assert not np.array_equal(_bits(h.cpu().numpy()), _bits(actor.History().transpose(1, 2, 0)))
