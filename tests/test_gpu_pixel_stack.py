"""GPU checks of the pixel frame stacks (gym.net_amd/csrc/pixel_stack.hip, gymnet_vecenv_pixel_stack_*): every slot equals what
gymnet_vecenv_render_device draws, bit for bit, for float32 and float64 handles, edge states, odd sizes and unaligned / padded strides; the
binary formats are (gray < 255); a closed auto-reset loop with truncations matches the NumPy model (tests/_pixel_stack_model.py) after every
push; explicit done bytes, handles without auto-reset and masked resets; no side effects on the env; the twin's geometry; refused calls
write nothing; the Python façade."""
import ctypes as C

import numpy as np
import pytest

import _pixel_stack_model as model
import _render_twin as twin

pytestmark = pytest.mark.gpu
SEED = 0x5EED
GRAY8, BINARY8, BINARY_F32 = model.GRAY8, model.BINARY8, model.BINARY_F32
RUNNER = ((200, 150, 200, 150), (40, 20))
SHAPES = [RUNNER, ((0, 0, 600, 400), (84, 84)), ((0, 0, 600, 400), (7, 5)), ((100, 50, 300, 250), (33, 17))]


def _edge_states(dtype, n_random=0):
    xs = [0.0, 1.2, -1.2, 2.4, -2.4, 3.0, -3.0]
    ths = [0.0, 0.2, -0.2, np.pi / 2, -np.pi / 2, np.pi, 7.0]
    rows = [(x, t) for x in xs for t in ths]
    rows += [(np.nan, 0.0), (np.inf, 0.1), (-np.inf, 0.0), (0.5, np.nan), (-0.5, np.inf), (0.0, -np.inf), (np.nan, np.nan)]
    rng = np.random.default_rng(5)
    rows += [(rng.uniform(-2.6, 2.6), rng.uniform(-0.5, 0.5)) for _ in range(n_random)]
    s = np.zeros((4, len(rows)), dtype)
    s[0] = [r[0] for r in rows]
    s[2] = [r[1] for r in rows]
    s[1], s[3] = 0.3, -0.7
    return s


def _config(env, fmt, depth, crop, size, ext=None, stride=0):
    return env._lib.gymnet_vecenv_pixel_stack_config(env._h, fmt, depth, *crop, *size, None if ext is None else C.c_void_p(ext), stride)


def _read(env, fmt, depth, size, first=0, count=None):
    count = env.NumberOfEnvironments - first if count is None else count
    out = np.empty((count, depth, size[1], size[0]), np.float32 if fmt == BINARY_F32 else np.uint8)
    assert env._lib.gymnet_vecenv_pixel_stack_read(env._h, out.ctypes.data_as(C.c_void_p), first, count) == 0
    return out


def _gray(env, crop, size):
    """RenderDevice("gray") of every lane: uint8 [N, h, w]."""
    import torch
    n = env.NumberOfEnvironments
    out = torch.empty((n, size[1], size[0]), dtype=torch.uint8, device="cuda")
    env.RenderDevice(out, "gray", crop=crop, size=size)
    env.Sync()
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gray8_slots_equal_the_render_bitwise(gpu_pkg, dtype):
    s = _edge_states(dtype, n_random=200)
    n = s.shape[1]
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, dtype=dtype) as env:
        env.Reset()
        env.SetState(s)
        for crop, size in SHAPES:
            want = _gray(env, crop, size)
            depth = 3
            assert _config(env, GRAY8, depth, crop, size) == 0
            got = _read(env, GRAY8, depth, size)
            for k in range(depth):
                assert np.array_equal(got[:, k], want), (crop, size, k)
            # an adopted buffer at an odd offset with a padded lane stride: the same slots, the gaps keep their sentinel
            import torch
            frame = size[0] * size[1]
            stride = depth * frame + 5
            buf = torch.full((n * stride + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()                                      # torch's stream fills; the handle's does not wait for it
            assert _config(env, GRAY8, depth, crop, size, ext=buf.data_ptr() + 3, stride=stride) == 0
            env.Sync()
            b = buf.cpu().numpy()
            lanes = b[3:3 + n * stride].reshape(n, stride)
            assert np.array_equal(lanes[:, :depth * frame].reshape(n, depth, size[1], size[0]), np.repeat(want[:, None], depth, 1))
            assert (lanes[:, depth * frame:] == 0xA5).all() and (b[:3] == 0xA5).all() and (b[3 + n * stride:] == 0xA5).all()
            assert np.array_equal(_read(env, GRAY8, depth, size), got)
            assert _config(env, GRAY8, 0, crop, size) == 0


def test_binary_formats_are_gray_below_255(gpu_pkg):
    s = _edge_states(np.float32, n_random=300)
    n = s.shape[1]
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED) as env:
        env.Reset()
        env.SetState(s)
        for crop, size in SHAPES:
            g = _gray(env, crop, size)
            for fmt in (BINARY8, BINARY_F32):
                assert _config(env, fmt, 2, crop, size) == 0
                got = _read(env, fmt, 2, size)
                want = model.process(g, fmt)
                assert got.dtype == want.dtype
                assert np.array_equal(got, np.repeat(want[:, None], 2, 1)), (fmt, crop, size)
                assert got.view(np.uint8 if fmt == BINARY8 else np.uint32).tobytes() == np.repeat(want[:, None], 2, 1).tobytes()


@pytest.mark.parametrize("depth", [1, 2, 4])
def test_closed_loop_with_truncations_matches_the_model(gpu_pkg, depth):
    import torch
    n, steps = 4096, 200
    crop, size = RUNNER
    rng = np.random.default_rng(depth)
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=13) as env:
        env.Reset()
        st = env.PixelStack(depth=depth, size=size, crop=crop, format="gray8")
        m = model.PixelStackModel(_gray(env, crop, size), depth)
        env.Sync()
        assert np.array_equal(st.Tensor.cpu().numpy(), m.stack)
        isolated = truncated = 0
        for t in range(steps):
            acts = torch.from_numpy(rng.integers(0, 2, n).astype(np.int32)).cuda()
            st.Step(acts)
            done = env.GetArray("done")
            m.push(_gray(env, crop, size), done)
            assert np.array_equal(st.Tensor.cpu().numpy(), m.stack), t
            d = done != 0
            isolated += int((d[1:-1] & ~d[:-2] & ~d[2:]).sum())      # a lane finishing while both neighbours go on
            truncated += int((d & (env.GetArray("finished_length") == 13)).sum())
        assert isolated > 0 and truncated > 0


@pytest.mark.parametrize("fmt", ["gray8", "binary_f32"])
def test_deep_stacks_and_odd_sizes_shift_like_the_model(gpu_pkg, fmt):
    """Stacks deeper than the slots the kernel loads ahead of its shading (the rest move one at a time after it), and frames whose
    slots are not 16-byte aligned (7 x 5), through pushes with restarts."""
    import torch
    n = 300
    rng = np.random.default_rng(13)
    code = {"gray8": GRAY8, "binary_f32": BINARY_F32}[fmt]
    cases = [(((0, 0, 600, 400), (7, 5)), 6), (RUNNER, 6), (RUNNER, 64), (((100, 50, 300, 250), (33, 17)), 5)]
    for (crop, size), depth in cases:
        with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=4) as env:
            env.Reset()
            st = env.PixelStack(depth=depth, size=size, crop=crop, format=fmt)
            m = model.PixelStackModel(_gray(env, crop, size), depth, code)
            for t in range(depth + 3):
                a = torch.from_numpy(rng.integers(0, 2, n).astype(np.int32)).cuda()
                st.Step(a)
                m.push(_gray(env, crop, size), env.GetArray("done"))
                assert np.array_equal(st.Read(), m.stack), (size, depth, t)


def test_explicit_done_no_autoreset_and_masked_reset(gpu_pkg):
    import torch
    n = 2048
    crop, size = RUNNER
    rng = np.random.default_rng(9)
    s = np.stack([rng.uniform(-2.6, 2.6, n), rng.uniform(-2, 2, n), rng.uniform(-0.23, 0.23, n), rng.uniform(-2, 2, n)]).astype(np.float32)
    a = torch.from_numpy(rng.integers(0, 2, n).astype(np.int32)).cuda()
    # an explicit d_done overrides the handle's own done bytes
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True) as env:
        env.Reset()
        env.SetState(s)
        st = env.PixelStack(depth=3, size=size, crop=crop, format="binary8")
        m = model.PixelStackModel(_gray(env, crop, size), 3, BINARY8)
        env.StepDevice(a)
        own = env.GetArray("done")
        mine = (np.arange(n) % 3 == 0).astype(np.uint8)
        assert own.any() and not np.array_equal(own != 0, mine != 0)
        d_mine = torch.from_numpy(mine).cuda()             # kept alive: the push reads it on the handle's stream
        st.Push(d_mine)
        m.push(_gray(env, crop, size), mine)
        assert np.array_equal(st.Read(), m.stack)
        env.StepDevice(a)
        st.Push()                                        # the handle's own done bytes
        m.push(_gray(env, crop, size), env.GetArray("done"))
        assert np.array_equal(st.Read(), m.stack)
    # without AUTORESET and d_done = NULL no lane restarts, though some are done
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=False) as env:
        env.Reset()
        env.SetState(s)
        st = env.PixelStack(depth=2, size=size, crop=crop, format="gray8")
        m = model.PixelStackModel(_gray(env, crop, size), 2)
        env.StepDevice(a)
        done = env.GetArray("done")
        assert done.any()
        st.Push()
        m.push(_gray(env, crop, size))
        assert np.array_equal(st.Read(), m.stack)
        # ResetWhere(mask) + reset_device(mask) refill only the masked lanes
        mask = (done != 0).astype(np.uint8)
        env.ResetWhere(mask)
        d_mask = torch.from_numpy(mask).cuda()
        st.Reset(d_mask)
        m.reset(_gray(env, crop, size), mask)
        got = st.Read()
        assert np.array_equal(got, m.stack)
        k = np.flatnonzero(mask)
        assert np.array_equal(got[k, 0], got[k, 1]) and not np.array_equal(got[~(mask != 0), 0], got[~(mask != 0), 1])


def test_pushes_change_nothing_but_the_stack(gpu_pkg):
    import torch
    n = 4096
    rng = np.random.default_rng(3)
    acts = [torch.from_numpy(rng.integers(0, 2, n).astype(np.int32)).cuda() for _ in range(40)]
    masks = [torch.from_numpy(rng.integers(0, 2, n).astype(np.uint8)).cuda() for _ in range(40)]
    outs = []
    for push in (False, True):
        with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True, done_list=True, episode_stats=True, max_episode_steps=25) as env:
            env.Reset()
            if push:
                st = env.PixelStack(depth=4, format="binary_f32")
            for a, mask in zip(acts, masks):
                env.StepDevice(a)
                if push:
                    st.Push()
                    st.Reset(mask)
            env.Sync()
            ep = env.EpisodeStats()
            outs.append([env.GetState(), env.GetArray("reward"), env.GetArray("done"), env.Tick, env.Counters(),
                         env.GetArray("episode_return"), env.GetArray("episode_length"), ep[0], ep[1], np.sort(env.DoneLanes())])
    for x, y in zip(*outs):
        if isinstance(x, dict):
            assert x == y
        else:
            assert np.array_equal(np.asarray(x), np.asarray(y))


def test_binary_stack_matches_the_twin_geometry(gpu_pkg):
    n = 4096
    crop, size = RUNNER
    rng = np.random.default_rng(17)
    s = np.stack([rng.uniform(-2.6, 2.6, n), np.zeros(n), rng.uniform(-0.5, 0.5, n), np.zeros(n)]).astype(np.float32)
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED) as env:
        env.Reset()
        env.SetState(s)
        st = env.PixelStack(depth=2, size=size, crop=crop, format="binary8")
        got = st.Read()
        state = env.GetState()
    sub = np.arange(0, n, 8)
    want, amb = twin.render(state[0, sub], state[2, sub], twin.GRAY8, crop, size)
    sure = amb == 0
    for slot in range(2):
        b = got[sub, slot]
        assert np.array_equal(b[sure], (want[..., 0] < 255)[sure].astype(np.uint8))
    assert sure.mean() > 0.99


def test_refused_calls_write_nothing(gpu_pkg):
    import torch
    n = 64
    crop, size = RUNNER
    E = gpu_pkg._capi
    with gpu_pkg.VectorEnv("Pendulum-v1", 4, seed=SEED) as env:
        env.Reset()
        buf = torch.full((4 * 1600,), 0x5A, dtype=torch.uint8, device="cuda")
        assert _config(env, GRAY8, 2, crop, size, ext=buf.data_ptr()) == E.ERR_UNSUPPORTED
        env.Sync()
        assert (buf.cpu().numpy() == 0x5A).all()
        with pytest.raises(NotImplementedError):
            env.PixelStack()
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED) as env:
        env.Reset()
        out = np.full(n * 1600, 0x5A, np.uint8)
        p = out.ctypes.data_as(C.c_void_p)
        # before a stack is configured
        assert env._lib.gymnet_vecenv_pixel_stack_reset_device(env._h, None) == E.ERR_INVALID_ARG
        assert env._lib.gymnet_vecenv_pixel_stack_push_device(env._h, None) == E.ERR_INVALID_ARG
        assert env._lib.gymnet_vecenv_pixel_stack_view(env._h, None, None, None) == E.ERR_INVALID_ARG
        assert env._lib.gymnet_vecenv_pixel_stack_read(env._h, p, 0, n) == E.ERR_INVALID_ARG
        assert (out == 0x5A).all()
        assert _config(env, GRAY8, 2, crop, size) == 0
        before = _read(env, GRAY8, 2, size)
        d0, ls0, fb0 = C.c_void_p(), C.c_int64(), C.c_int64()
        assert env._lib.gymnet_vecenv_pixel_stack_view(env._h, C.byref(d0), C.byref(ls0), C.byref(fb0)) == 0
        assert (ls0.value, fb0.value) == (1600, 800)
        env.SetState(np.zeros((4, n), np.float32))           # the current frame now differs from the stack's
        buf = torch.full((n * 6400 + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        good = dict(fmt=GRAY8, depth=2, crop=crop, size=size, off=0, stride=0)
        bad = [dict(fmt=0), dict(fmt=1), dict(fmt=5), dict(depth=-1), dict(depth=65), dict(crop=(-1, 150, 200, 150)),
               dict(crop=(401, 150, 200, 150)), dict(crop=(200, 150, 0, 150)), dict(size=(0, 20)), dict(size=(40, 16385)),
               dict(stride=1599), dict(stride=-1600), dict(stride=1 << 62), dict(fmt=BINARY_F32, off=2), dict(fmt=BINARY_F32, stride=6402)]
        for b in bad:
            a = {**good, **b}
            assert _config(env, a["fmt"], a["depth"], a["crop"], a["size"], ext=buf.data_ptr() + a["off"], stride=a["stride"]) \
                == E.ERR_INVALID_ARG, b
        assert env._lib.gymnet_vecenv_pixel_stack_read(env._h, p, -1, 2) == E.ERR_INVALID_ARG
        assert env._lib.gymnet_vecenv_pixel_stack_read(env._h, p, n - 1, 2) == E.ERR_INVALID_ARG
        assert env._lib.gymnet_vecenv_pixel_stack_read(env._h, p, 0, 0) == E.ERR_INVALID_ARG
        assert env._lib.gymnet_vecenv_pixel_stack_read(env._h, None, 0, 1) == E.ERR_INVALID_ARG
        env.Sync()
        assert (buf.cpu().numpy() == 0x5A).all() and (out == 0x5A).all()
        d1, ls1, fb1 = C.c_void_p(), C.c_int64(), C.c_int64()
        assert env._lib.gymnet_vecenv_pixel_stack_view(env._h, C.byref(d1), C.byref(ls1), C.byref(fb1)) == 0
        assert (d1.value, ls1.value, fb1.value) == (d0.value, 1600, 800)
        assert np.array_equal(_read(env, GRAY8, 2, size), before)
        # the good request itself works
        assert _config(env, GRAY8, 2, crop, size, ext=buf.data_ptr()) == 0
        env.Sync()
        assert (buf.cpu().numpy()[:n * 1600] != 0x5A).any()
        assert _config(env, GRAY8, 0, crop, size) == 0            # released: calls are refused again
        assert env._lib.gymnet_vecenv_pixel_stack_push_device(env._h, None) == E.ERR_INVALID_ARG


@pytest.mark.parametrize("fmt,dt", [("gray8", "uint8"), ("binary8", "uint8"), ("binary_f32", "float32")])
def test_python_facade(gpu_pkg, fmt, dt):
    import torch
    n = 1000
    rng = np.random.default_rng(21)
    acts = [torch.from_numpy(rng.integers(0, 2, n).astype(np.int32)).cuda() for _ in range(30)]
    tensors = []
    for via_step in (True, False):
        with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True, dtype=np.float64) as env:
            env.Reset()
            st = env.PixelStack(depth=3, size=(21, 13), crop=(150, 100, 300, 250), format=fmt)
            assert tuple(st.Tensor.shape) == (n, 3, 13, 21) and st.Tensor.dtype == getattr(torch, dt)
            for a in acts:
                if via_step:
                    st.Step(a)
                else:
                    env.StepDevice(a)
                    st.Push()
            env.Sync()
            host = st.Read()
            assert host.dtype == np.dtype(dt) and np.array_equal(host, st.Tensor.cpu().numpy())
            assert np.array_equal(st.Read(lanes=(7, 5)), host[7:12])
            tensors.append(host)
            # a caller's tensor with padded lanes is adopted with its stride(0)
            big = torch.zeros((n, 4, 13, 21), dtype=getattr(torch, dt), device="cuda")
            torch.cuda.synchronize()                               # the zeros are in place before the handle's stream writes
            st2 = env.PixelStack(depth=3, size=(21, 13), crop=(150, 100, 300, 250), format=fmt, out=big[:, :3])
            env.Sync()
            assert (big[:, 3] == 0).all() and np.array_equal(big[:, :3].cpu().numpy(), st2.Read())
            with pytest.raises(ValueError):
                st.Push()                                          # replaced by st2
            st2.Close()
            with pytest.raises(ValueError):
                st2.Push()
    assert np.array_equal(tensors[0], tensors[1])
