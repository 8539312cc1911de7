"""GPU checks of the three frame kernels — render_kernel (render.hip), pixel_stack_kernel (pixel_stack.hip) and memory_frames_kernel
(episode_memory.hip), which share one rasteriser (cartpole_raster.hpp) — against the float64 twin (tests/_render_twin.py) at every
geometry of tests/_raster_geometry_cases.py: unambiguous pixels exactly, a pixel with k samples within 1e-3 px of an edge within
ceil(255 k / 16).  Which case reaches which path of the kernels is the third column of that table:

  frames shorter than a thread's 16 pixels (byte tail; dword tail for BINARY_F32)   1x1, 5x3
  out_w < 16, the row wrap inside a thread; out_w = 1                               5x3, 1x37, tall
  ragged last wave, odd frame_bytes with packed frames (dwordx4 / byte alternate)   17x61 (and 5x3, 1x37, odd)
  RGB8 away from 600 x 400                                                          every case
  non-integer ratios, upscaling (sxq < 0.25), the 16384 limit                       84x84, odd, 160x210; up4, up32; wide, tall
  horizontal / inverted poles under a crop, theta beyond 65536                      every cropped case: the state set holds them
  carts far off the canvas, cx overflowing float32, signed zeros, subnormals        every case: the state set holds them
  the second trip of each kernel's grid-stride loop                                 the three test_second_trip_* tests

The state set (cases.states) is the 56 edge rows of test_gpu_render.py, 40 random lanes over x in (-2.6, 2.6) and theta in (-pi, pi),
and the rows named there; a case above 50 000 pixels uses its first 24 lanes."""
import ctypes as C

import numpy as np
import pytest

import _pixel_stack_model as model
import _raster_geometry_cases as cases
import _render_twin as twin

pytestmark = pytest.mark.gpu
SEED = 0x5EED
RGB8, GRAY8 = twin.RGB8, twin.GRAY8
FMT_NAME = {RGB8: "rgb", GRAY8: "gray"}
STACK = {"gray8": model.GRAY8, "binary8": model.BINARY8, "binary_f32": model.BINARY_F32}
DATASET_CASES = ("5x3", "17x61")


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _sentinel(nbytes):
    """A device buffer of 0xA5 bytes.  torch fills it on ITS stream and the handle's stream does not wait for that one, so the fill is
    finished here, before any kernel of the handle can write into the buffer."""
    import torch
    t = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def handles(gpu_pkg):
    """One CartPole handle per (dtype, lane count of a case), holding cases.states: made on first use, closed with the module."""
    made = {}

    def get(dtype, name):
        s = cases.states(dtype, name)
        key = (np.dtype(dtype).name, s.shape[1])
        if key not in made:
            env = gpu_pkg.VectorEnv("CartPole-v1", s.shape[1], seed=SEED, dtype=dtype)
            env.Reset()
            env.SetState(s)
            got = env.GetState()
            assert got.dtype == s.dtype and got.tobytes() == s.tobytes()        # the handle holds the rows bit for bit, NaN and -0.0 too
            made[key] = env
        return made[key], s
    yield get
    for env in made.values():
        env.Close()


def _render_both(env, fmt, crop, size, stride, offset=0, tail=0):
    """The host call and the device call for every lane, into sentinel-filled buffers of n * stride + tail bytes starting `offset`
    bytes in: (host bytes, device bytes)."""
    n = env.NumberOfEnvironments
    host = np.full(offset + n * stride + tail, 0xA5, np.uint8)
    assert env._lib.gymnet_vecenv_render(env._h, C.c_void_p(host.ctypes.data + offset), fmt, 0, n, *crop, *size, stride) == 0
    dev = _sentinel(offset + n * stride + tail)
    env.RenderDevice(dev.data_ptr() + offset, FMT_NAME[fmt], crop=crop, size=size, lane_stride=stride)
    env.Sync()
    return host, dev.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("fmt", [RGB8, GRAY8], ids=["rgb8", "gray8"])
@pytest.mark.parametrize("name", cases.NAMES)
def test_render_equals_the_twin(handles, name, fmt, dtype):
    """Render (host) and RenderDevice with lane_stride == frame_bytes: frames back to back, so a frame of odd size starts at every
    alignment and the lanes alternate between the kernel's dwordx4 path and its byte path."""
    env, s = handles(dtype, name)
    crop, (w, h) = cases.crop_size(name)
    n, ch = s.shape[1], 3 if fmt == RGB8 else 1
    frame = w * h * ch
    host, dev = _render_both(env, fmt, crop, (w, h), frame, tail=64)
    assert (host[n * frame:] == 0xA5).all()
    assert np.array_equal(host, dev)
    t = cases.truth(name, dtype)
    share = twin.compare(host[:n * frame].reshape(n, h, w, ch), t[fmt], t["amb"])
    print(f"{name}: {n} lanes, ambiguous share {share:.5f}")
    assert share <= cases.AMBIGUOUS_CAP


@pytest.mark.parametrize("name", cases.NAMES)
def test_render_with_a_padded_stride_keeps_the_sentinel(handles, name):
    """lane_stride = frame_bytes + 5 from an odd offset, RGB8, float32: the frames equal the twin, the 5 bytes after each frame, the
    bytes before the first and the bytes past the last keep their sentinel — in the device call's buffer and the host call's."""
    env, s = handles(np.float32, name)
    crop, (w, h) = cases.crop_size(name)
    n, frame = s.shape[1], w * h * 3
    stride = frame + 5
    host, dev = _render_both(env, RGB8, crop, (w, h), stride, offset=3, tail=59)
    assert np.array_equal(host, dev)
    lanes = dev[3:3 + n * stride].reshape(n, stride)
    assert (lanes[:, frame:] == 0xA5).all() and (dev[:3] == 0xA5).all() and (dev[3 + n * stride:] == 0xA5).all()
    t = cases.truth(name, np.float32)
    twin.compare(lanes[:, :frame].reshape(n, h, w, 3), t[RGB8], t["amb"])


@pytest.mark.parametrize("depth,dtype", [(2, np.float32), (5, np.float64)], ids=["depth2-f32", "depth5-f64"])
@pytest.mark.parametrize("fmt", list(STACK))
@pytest.mark.parametrize("name", cases.SMALL)
def test_pixel_stack_slots_equal_the_twin(handles, name, fmt, depth, dtype):
    """Every slot after config and after each of three pushes with a restart mask, against the twin frame of the state the slot was drawn
    from: GRAY8 through twin.compare, the binary formats exactly on pixels without an ambiguous sample.  Which state a slot holds comes
    from tests/_pixel_stack_model.py fed with the TWIN's frames (and, in a second instance, the twin's ambiguity counts).  Between pushes
    the lanes' states rotate through the case's state set, so the twin frames are the shared ones.  Depth 5 is beyond the three older
    slots the kernel loads ahead of its shading; depth 2 runs on a float32 handle, depth 5 on a float64 one."""
    env, s = handles(dtype, name)
    crop, (w, h) = cases.crop_size(name)
    n = s.shape[1]
    t = cases.truth(name, dtype)
    gray, amb = t[GRAY8][..., 0], t["amb"].astype(np.uint8)                 # at most 16 samples per pixel
    rng = np.random.default_rng(depth)
    st = None
    try:
        st = env.PixelStack(depth=depth, size=(w, h), crop=crop, format=fmt)
        want, unsure = model.PixelStackModel(gray, depth, STACK[fmt]), model.PixelStackModel(amb, depth)
        for push in range(4):
            if push:
                order = np.roll(np.arange(n), 7 * push)                      # lane k now holds state order[k] of the set
                env.SetState(np.ascontiguousarray(s[:, order]))
                done = (rng.random(n) < 0.3).astype(np.uint8)
                d_done = _dev(done)                                          # kept alive: the push reads it on the handle's stream
                st.Push(d_done)
                want.push(gray[order], done)
                unsure.push(amb[order], done)
            got = st.Read()
            assert got.shape == want.stack.shape and got.dtype == want.stack.dtype
            if fmt == "gray8":
                twin.compare(got.reshape(n * depth, h, w, 1), want.stack.reshape(n * depth, h, w, 1),
                             unsure.stack.reshape(n * depth, h, w).astype(np.int64))
            else:
                sure = unsure.stack == 0
                assert np.array_equal(got[sure], want.stack[sure]), (push, int((got[sure] != want.stack[sure]).sum()))
                assert set(np.unique(got)) <= {0, 1}
    finally:
        env.SetState(s)
        if st is not None:
            st.Close()


# ---- dataset frames ------------------------------------------------------------------------------------------------------------

def _fill_memory(gpu_pkg, history, capacity, steps, max_steps):
    """A float32 CartPole handle of 1024 lanes stepped with random actions, every step pushed into an episode memory."""
    n = 1024
    rng = np.random.default_rng(history)
    env = gpu_pkg.VectorEnv("CartPole-v1", n, seed=SEED, auto_reset=True, episode_stats=True, max_episode_steps=max_steps)
    env.Reset()
    mem = env.EpisodeMemory(capacity=capacity, max_length=0, history=history)
    for _ in range(steps):
        a = _dev(rng.integers(0, 2, n).astype(np.int32))
        env.StepDevice(a)
        mem.Push(a)
        env.Sync()
    assert mem.Stats()["kept"] == capacity
    return env, mem


def _frame_states(mem, history):
    """(x, theta) float32 [rows, history] of every dataset frame, from the "params" dataset of the same memory: a row's own state is the
    newest entry of its params row; frame s of row p of an episode shows the episode's row max(p - (history - 1) + s, 0), as the kernel
    clamps q.  The episodes' rows come from Episodes(): length * 2 // 3 each, in the dataset's order."""
    x, _, _ = mem.BuildDataset("params", min_episodes=0)
    x = x.cpu().numpy().reshape(-1, history, 4)
    own = x[:, history - 1]
    _, length, _, _ = mem.Episodes()
    per = length.astype(np.int64) * 2 // 3
    assert per.sum() == len(own) == mem.DatasetSize()
    first = np.repeat(np.cumsum(per) - per, per)                             # the first dataset row of each row's episode
    p = np.arange(len(own)) - first
    q = np.maximum(p[:, None] - (history - 1) + np.arange(history)[None, :], 0)
    src = own[first[:, None] + q]                                            # [rows, history, 4]
    assert np.array_equal(src, x)                                            # the params dataset clamps the same way
    return src[..., 0], src[..., 2]


@pytest.fixture(scope="module")
def memories(gpu_pkg):
    made = {}

    def get(history):
        if history not in made:
            made[history] = _fill_memory(gpu_pkg, history, capacity=48, steps=100, max_steps=30)
        return made[history]
    yield get
    for env, _ in made.values():
        env.Close()


@pytest.mark.parametrize("history", [1, 4])
@pytest.mark.parametrize("name", DATASET_CASES)
def test_dataset_frames_equal_the_twin(memories, name, history):
    """BuildDataset in the three pixel formats at 5x3 (a frame shorter than a thread's 16 pixels) and 17x61 (a second wave of 13 pixels,
    odd frame_bytes), history 1 and 4, on a fixed subset of 300 rows that holds the first rows of episodes (where q is clamped)."""
    env, mem = memories(history)
    crop, (w, h) = cases.crop_size(name)
    x, th = _frame_states(mem, history)
    rows = len(x)
    _, length, _, _ = mem.Episodes()
    per = length.astype(np.int64) * 2 // 3
    starts = (np.cumsum(per) - per)[per > 0]
    sub = np.unique(np.concatenate([starts[:40], starts[:40] + 1, np.random.default_rng(5).choice(rows, 220, replace=False), [rows - 1]]))
    sub = sub[sub < rows]
    _, gray, amb = cases.frames_of(x[sub].reshape(-1), th[sub].reshape(-1), crop, (w, h))
    gray, amb = gray.reshape(len(sub), history, h, w), amb.reshape(len(sub), history, h, w)
    assert (gray < 255).any() and (gray == 255).any()
    for fmt, code in STACK.items():
        got = mem.BuildDataset(fmt, size=(w, h), crop=crop, min_episodes=0)[0].cpu().numpy()
        assert got.shape == (rows, history, h, w)
        if fmt == "gray8":
            twin.compare(got[sub].reshape(-1, h, w, 1), gray.reshape(-1, h, w, 1), amb.reshape(-1, h, w))
        else:
            want = model.process(gray, code)
            assert got.dtype == want.dtype
            assert np.array_equal(got[sub][amb == 0], want[amb == 0]), fmt
    assert (amb > 0).mean() <= cases.AMBIGUOUS_CAP


# ---- the second trip of each grid-stride loop ----------------------------------------------------------------------------------

BIG_N = (1 << 22) + 77
RENDER_GRID_WAVES = 4 << 20          # launch_render_typed / launch_pixel_stack_typed: at most 2^20 workgroups of 4 waves
MEMORY_GRID_WAVES = 4 << 16          # launch_dataset_typed: at most 2^16 workgroups of 4 waves


def _big_states(seed):
    rng = np.random.default_rng(seed)
    s = np.zeros((4, BIG_N), np.float32)
    s[0] = rng.uniform(-2.6, 2.6, BIG_N)
    s[2] = rng.uniform(-np.pi, np.pi, BIG_N)
    return s


@pytest.fixture(scope="module")
def big(gpu_pkg):
    """A CartPole handle of 2^22 + 77 lanes with random states, and its 1 x 1 GRAY8 frames of the whole canvas rendered in calls of at
    most 2^20 lanes (2^20 waves each: no call wraps its grid)."""
    s = _big_states(31)
    env = gpu_pkg.VectorEnv("CartPole-v1", BIG_N, seed=SEED)
    env.Reset()
    env.SetState(s)

    def chunked():
        out = _sentinel(BIG_N)
        for first in range(0, BIG_N, 1 << 20):
            count = min(1 << 20, BIG_N - first)
            assert count * cases.waves("1x1") <= RENDER_GRID_WAVES
            env.RenderDevice(out.data_ptr() + first, "gray", first_lane=first, count=count, crop=cases.CANVAS, size=(1, 1))
        env.Sync()
        return out.cpu().numpy()
    yield env, s, chunked
    env.Close()


def test_second_trip_of_the_render_loop(big):
    """2^22 + 77 one-pixel frames in ONE call: 2^22 + 77 waves on a grid of 2^22, so 77 waves are a second trip of render_kernel's loop.
    Byte for byte the frames of calls that cannot wrap, and the twin's on the first and last 4096 lanes, the 200 around 2^22 and every
    61st lane."""
    env, s, chunked = big
    assert BIG_N * cases.waves("1x1") > RENDER_GRID_WAVES
    out = _sentinel(BIG_N + 64)
    env.RenderDevice(out, "gray", crop=cases.CANVAS, size=(1, 1))
    env.Sync()
    got = out.cpu().numpy()
    assert (got[BIG_N:] == 0xA5).all()
    assert np.array_equal(got[:BIG_N], chunked())
    sub = np.unique(np.concatenate([np.arange(4096), np.arange(BIG_N - 4096, BIG_N), np.arange((1 << 22) - 100, (1 << 22) + 77),
                                    np.arange(0, BIG_N, 61)]))
    _, want, amb = cases.frames_of(s[0, sub], s[2, sub], cases.CANVAS, (1, 1))
    assert (want == 255).any() and (want < 255).any()                          # one pixel of the whole canvas: few lanes put a shape on a sample
    twin.compare(got[sub].reshape(-1, 1, 1, 1), want, amb)


def test_second_trip_of_the_pixel_stack_loop(big):
    """PixelStack(depth=2, size=(1, 1), format="binary8") on the same handle: the config and one push with a restart mask each run
    2^22 + 77 waves on a grid of 2^22.  A lane that restarts holds the new frame twice, every other lane the old and the new one, both
    from the chunked render."""
    env, s, chunked = big
    assert BIG_N * cases.waves("1x1") > RENDER_GRID_WAVES
    st = None
    try:
        old = (chunked() < 255).astype(np.uint8)
        st = env.PixelStack(depth=2, size=(1, 1), crop=cases.CANVAS, format="binary8")
        env.Sync()
        assert np.array_equal(st.Tensor.cpu().numpy().reshape(BIG_N, 2), np.stack([old, old], 1))
        env.SetState(_big_states(32))
        new = (chunked() < 255).astype(np.uint8)
        done = (np.random.default_rng(33).random(BIG_N) < 0.4).astype(np.uint8)
        d_done = _dev(done)
        st.Push(d_done)
        env.Sync()
        got = st.Tensor.cpu().numpy().reshape(BIG_N, 2)
        assert np.array_equal(got[:, 1], new)
        assert np.array_equal(got[:, 0], np.where(done != 0, new, old))
        tail = slice(1 << 22, BIG_N)                                          # the second trip's lanes see both kinds
        assert done[tail].any() and not done[tail].all() and old.any() and new.any() and (old != new).any()
    finally:
        env.SetState(s)
        if st is not None:
            st.Close()


def test_second_trip_of_the_dataset_frames_loop(gpu_pkg):
    """history = 64, 1 x 1 binary8 frames, more than 4096 dataset rows: rows * 64 waves on a grid of 4 * 2^16, so memory_frames_kernel's
    loop takes further trips.  The crop (280, 230, 40, 40) puts the four sample columns across an upright pole at the centre, so frames
    of both values occur.  Every frame against the twin of its params row."""
    crop, size, history = (280, 230, 40, 40), (1, 1), 64
    env, mem = _fill_memory(gpu_pkg, history, capacity=400, steps=120, max_steps=40)
    try:
        x, th = _frame_states(mem, history)
        rows = len(x)
        assert rows > 4096 and rows * history * 1 > MEMORY_GRID_WAVES
        got = mem.BuildDataset("binary8", size=size, crop=crop, min_episodes=0)[0].cpu().numpy()
        assert got.shape == (rows, history, 1, 1)
        _, gray, amb = cases.frames_of(x.reshape(-1), th.reshape(-1), crop, size)
        want = model.process(gray.reshape(rows, history, 1, 1), model.BINARY8)
        sure = amb.reshape(rows, history, 1, 1) == 0
        assert np.array_equal(got[sure], want[sure])
        # a frame is ONE pixel here: its 4 x 4 samples lie across the pole, whose two long edges pass a sample column whenever the cart
        # moves by a few pixels (4 columns x 2 edges x 4 rows x 2 EPS over the ~20 px the carts spread: about 0.003 of the frames), so
        # the table's cap per pixel does not apply; the bound is test_gpu_pixel_stack.py's for the binary stack against the twin
        assert sure.mean() > 0.99 and want[sure].any() and not want[sure].all()
    finally:
        env.Close()
