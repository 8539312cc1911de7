"""GPU checks of CartPole rendering (gym.net_amd/csrc/render.hip): frames against the NumPy twin (tests/_render_twin.py) — unambiguous
pixels exactly, pixels with a sample within 1e-3 px of an edge within ceil(255 k / 16) — for float32 and float64 handles, the Images
runner's stacked GRAY8 layout, argument validation (nothing written), no side effects, stream ordering, and the façades."""
import ctypes as C

import numpy as np
import pytest

import _render_twin as twin

pytestmark = pytest.mark.gpu
SEED = 0x5EED
RGB8, GRAY8 = twin.RGB8, twin.GRAY8
CANVAS = (0, 0, 600, 400)


def _edge_states(dtype):
    xs = [0.0, 1.2, -1.2, 2.4, -2.4, 3.0, -3.0]
    ths = [0.0, 0.2, -0.2, np.pi / 2, -np.pi / 2, np.pi, 7.0]
    rows = [(x, t) for x in xs for t in ths]
    rows += [(np.nan, 0.0), (np.inf, 0.1), (-np.inf, 0.0), (0.5, np.nan), (-0.5, np.inf), (0.0, -np.inf), (np.nan, np.nan)]
    s = np.zeros((4, len(rows)), dtype)
    s[0] = [r[0] for r in rows]
    s[2] = [r[1] for r in rows]
    s[1], s[3] = 0.3, -0.7
    return s


def _host_render(env, out, fmt, first, count, crop, size, stride, offset=0):
    return env._lib.gymnet_vecenv_render(env._h, C.c_void_p(out.ctypes.data + offset), fmt, first, count, *crop, *size, stride)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rgb8_full_frames_equal_the_twin(gpu_pkg, dtype):
    s = _edge_states(dtype)
    n = s.shape[1]
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, dtype=dtype) as env:
        env.Reset()
        env.SetState(s)
        got = env.Render("rgb_array", lanes=range(n))
        st = env.GetState()
    assert got.shape == (n, 400, 600, 3) and got.dtype == np.uint8
    want, amb = twin.render(st[0], st[2])
    frac = twin.compare(got, want, amb)
    assert frac < 0.01, frac
    assert (amb > 0).mean(axis=(1, 2)).max() < 0.01


def test_gray8_images_runner_layout(gpu_pkg):
    """2^16 random lanes, crop (200, 150, 200, 150) -> 40 x 20, written into the second half of 1600-byte slots (two frames stacked into
    one 40 x 40 input): the first halves and the bytes past the end keep their sentinel; host and device calls agree byte for byte,
    at an aligned and at an odd device offset."""
    import torch
    n = 1 << 16
    rng = np.random.default_rng(7)
    s = np.stack([rng.uniform(-2.6, 2.6, n), rng.uniform(-2, 2, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-2, 2, n)]).astype(np.float32)
    crop, size, stride = (200, 150, 200, 150), (40, 20), 1600
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED) as env:
        env.Reset()
        env.SetState(s)
        buf = np.full(n * stride + 64, 0xA5, np.uint8)
        assert _host_render(env, buf, GRAY8, 0, n, crop, size, stride, offset=800) == 0
        dev = torch.full((n * stride + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        odd = torch.full((n * stride + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()                                          # torch's stream fills; the handle's does not wait for it
        env.RenderDevice(dev.data_ptr() + 800, "gray", crop=crop, size=size, lane_stride=stride)
        env.RenderDevice(odd.data_ptr() + 801, "gray", crop=crop, size=size, lane_stride=stride)
        env.Sync()
        frames = env.RenderFrames(size, crop=crop)
        st = env.GetState()
    slots = buf[:n * stride].reshape(n, stride)
    assert (slots[:, :800] == 0xA5).all() and (buf[n * stride:] == 0xA5).all()
    assert np.array_equal(dev.cpu().numpy(), buf)
    o = odd.cpu().numpy()
    at = 801 + np.arange(n)[:, None] * stride + np.arange(800)[None, :]
    assert np.array_equal(o[at], slots[:, 800:])
    untouched = np.ones(o.shape, bool)
    untouched[at] = False
    assert (o[untouched] == 0xA5).all()
    assert np.array_equal(frames.reshape(n, 800), slots[:, 800:])
    sub = np.arange(0, n, 8)                                          # the twin is ~1 ms per lane: every eighth lane
    want, amb = twin.render(st[0, sub], st[2, sub], GRAY8, crop, size)
    frac = twin.compare(slots[sub, 800:].reshape(len(sub), 20, 40, 1), want, amb)
    assert frac < 0.01, frac


def test_lane_ranges_and_argument_validation(gpu_pkg):
    n = 64
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED) as env:
        env.Reset()
        full = env.RenderFrames((40, 20), crop=(200, 150, 200, 150))
        part = env.RenderFrames((40, 20), crop=(200, 150, 200, 150), lanes=(10, 5))
        assert np.array_equal(part, full[10:15])
        assert np.array_equal(env.RenderFrames((40, 20), crop=(200, 150, 200, 150), lanes=(n - 1, 1))[0], full[-1])
        good = dict(fmt=GRAY8, first=0, count=2, crop=(0, 0, 600, 400), size=(30, 20), stride=600)
        bad = [dict(fmt=0), dict(fmt=3), dict(first=-1), dict(first=n - 1, count=2), dict(count=0), dict(count=-1), dict(first=n, count=1),
               dict(crop=(-1, 0, 600, 400)), dict(crop=(0, -1, 600, 400)), dict(crop=(1, 0, 600, 400)), dict(crop=(0, 1, 600, 400)),
               dict(crop=(0, 0, 0, 400)), dict(crop=(0, 0, 600, 0)), dict(crop=(0, 0, -5, 400)), dict(size=(0, 20)), dict(size=(30, 0)),
               dict(size=(-1, 20)), dict(size=(16385, 1)), dict(stride=599), dict(fmt=RGB8, stride=1799)]
        buf = np.full(8192, 0x5A, np.uint8)
        import torch
        dev = torch.full((8192,), 0x5A, dtype=torch.uint8, device="cuda")
        for b in bad:
            a = {**good, **b}
            args = (a["fmt"], a["first"], a["count"], *a["crop"], *a["size"], a["stride"])
            assert env._lib.gymnet_vecenv_render(env._h, C.c_void_p(buf.ctypes.data), *args) == gpu_pkg._capi.ERR_INVALID_ARG, b
            assert env._lib.gymnet_vecenv_render_device(env._h, C.c_void_p(dev.data_ptr()), *args) == gpu_pkg._capi.ERR_INVALID_ARG, b
        a = good
        args = (a["fmt"], a["first"], a["count"], *a["crop"], *a["size"], a["stride"])
        assert env._lib.gymnet_vecenv_render(env._h, None, *args) == gpu_pkg._capi.ERR_INVALID_ARG
        assert env._lib.gymnet_vecenv_render_device(env._h, None, *args) == gpu_pkg._capi.ERR_INVALID_ARG
        env.Sync()
        assert (buf == 0x5A).all() and (dev.cpu().numpy() == 0x5A).all()
        with pytest.raises(ValueError):
            env.RenderFrames((40, 20), crop=(0, 0, 601, 400))
        # the good request itself works
        assert env._lib.gymnet_vecenv_render(env._h, C.c_void_p(buf.ctypes.data), *args) == 0 and (buf[:1200] != 0x5A).any()
    with gpu_pkg.VectorEnv("Pendulum-v1", 4, seed=SEED) as env:
        env.Reset()
        buf = np.full(4 * 600, 0x5A, np.uint8)
        assert env._lib.gymnet_vecenv_render(env._h, C.c_void_p(buf.ctypes.data), GRAY8, 0, 4, 0, 0, 600, 400, 30, 20, 600) \
            == gpu_pkg._capi.ERR_UNSUPPORTED
        assert (buf == 0x5A).all()
        with pytest.raises(NotImplementedError):               # GYMNET_ERR_UNSUPPORTED
            env.Render("rgb_array")


def test_rendering_has_no_side_effects(gpu_pkg):
    n = 4096
    rng = np.random.default_rng(3)
    s = np.stack([rng.uniform(-2.6, 2.6, n), rng.uniform(-2, 2, n), rng.uniform(-0.23, 0.23, n), rng.uniform(-2, 2, n)]).astype(np.float32)
    a = rng.integers(0, 2, n).astype(np.int32)
    outs = []
    for render in (False, True):
        with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True, done_list=True, episode_stats=True) as env:
            env.Reset()
            env.SetState(s)
            env.Step(a)
            if render:
                env.Render("rgb_array", lanes=[0, n - 1])
                env.RenderFrames((40, 20), crop=(200, 150, 200, 150))
            r = env.Step(a)
            outs.append((r.Observation, r.Reward, r.Done, env.Tick, env.Counters(), env.GetState(), env.EpisodeStats()))
    for x, y in zip(*outs):
        if isinstance(x, tuple):
            for u, v in zip(x, y):
                assert np.array_equal(u, v)
        elif isinstance(x, dict):
            assert x == y
        else:
            assert np.array_equal(x, y)


def test_stream_ordering_double_buffer_and_auto_reset(gpu_pkg):
    import torch
    n = 1024
    crop, size = (200, 150, 200, 150), (40, 20)
    rng = np.random.default_rng(11)
    s = np.stack([rng.uniform(-2.6, 2.6, n), rng.uniform(-2, 2, n), rng.uniform(-0.23, 0.23, n), rng.uniform(-2, 2, n)]).astype(np.float32)
    for double_buffer in (False, True):
        with gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True, double_buffer=double_buffer) as env:
            env.Reset()
            env.SetState(s)
            acts = torch.from_numpy(rng.integers(0, 2, n).astype(np.int32)).cuda()
            out = torch.full((n * 800,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()                                      # the sentinel is in place before the handle's stream starts
            for _ in range(3):
                env.StepDevice(acts)                               # no synchronize in between: the render is ordered after the step
            env.RenderDevice(out, "gray", crop=crop, size=size)
            env.Sync()
            st = env.GetState()
            done = env.GetArray("done")
            got = out.cpu().numpy().reshape(n, 20, 40, 1)
            want, amb = twin.render(st[0], st[2], GRAY8, crop, size)
            twin.compare(got, want, amb)
            # lanes that just finished show their reset state: GetState holds it, and a reset state is near the centre
            k = np.flatnonzero(done)
            assert len(k) and (np.abs(st[:, k]) <= 0.05).all()


@pytest.mark.parametrize("resident", [False, True])
def test_facades(gpu_pkg, resident):
    with gpu_pkg.CartPoleEnv(seed=SEED, resident=resident) as e:
        obs = e.Reset()
        frame = e.Render("rgb_array")
        assert e.Render() is None and e.Render("human") is None
        with pytest.raises(ValueError):
            e.Render("bogus")
        state = e._v.GetState()
    assert frame.shape == (400, 600, 3) and frame.dtype == np.uint8
    assert np.array_equal(state[:, 0], obs)
    with gpu_pkg.VectorEnv("CartPole-v1", 1, seed=SEED, dtype=np.float64) as v:
        v.Reset()
        v.SetState(state)
        assert np.array_equal(v.Render("rgb_array")[0], frame)
        assert v.Render() is None
        with pytest.raises(ValueError):
            v.Render("bogus")
    want, amb = twin.render(state[0], state[2])
    twin.compare(frame[None], want, amb)
