"""CPU checks of the pixel frame stacks (gymnet_vecenv_pixel_stack_*): the library exports the five calls, the header, ctypes and
Native.cs declare them with the same arity, the format enum is in every binding and every host wrapper reaches the calls, and the NumPy
model the GPU tests compare against (tests/_pixel_stack_model.py) shifts, restarts and masks as the contract says — on hand-worked
sequences and on the twin's frames of known states in the Images runner's layout (two 40 x 20 frames, the oldest on top)."""
import ctypes
import os
import re

import numpy as np

import _pixel_stack_model as model
import _render_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"gymnet_vecenv_pixel_stack_config": 11, "gymnet_vecenv_pixel_stack_reset_device": 2, "gymnet_vecenv_pixel_stack_push_device": 2,
         "gymnet_vecenv_pixel_stack_view": 4, "gymnet_vecenv_pixel_stack_read": 4}
CROP, SIZE = (200, 150, 200, 150), (40, 20)


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _arity(text, name):
    m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*[;{]" % name, text, flags=re.S)
    assert m, name
    args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
    return len(args)


def test_library_and_bindings_declare_the_stack_calls(gymnet):
    lib = ctypes.CDLL(gymnet.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", _read("include", "gymnet_amd.h"), flags=re.S)
    native = _read("gym.net_amd", "csharp", "Native.cs")
    for name, n in CALLS.items():
        assert hasattr(lib, name), name
        assert _arity(hdr, name) == n, name
        assert name in gymnet._capi.PROTOTYPES and len(gymnet._capi.PROTOTYPES[name][1]) == n, name
        assert re.search(r"\[DllImport\(Lib\)\] public static extern int %s\(" % name, native), name
        assert _arity(native, name) == n, name
    assert "enum { GYMNET_STACK_GRAY8 = 2, GYMNET_STACK_BINARY8 = 3, GYMNET_STACK_BINARY_F32 = 4 };" in hdr
    assert "enum { GYMNET_PIXELS_RGB8 = 1, GYMNET_PIXELS_GRAY8 = 2 };" in hdr
    assert "public enum GymnetStackFormat { Gray8 = 2, Binary8 = 3, BinaryF32 = 4 }" in native
    c = gymnet._capi
    assert (c.STACK_GRAY8, c.STACK_BINARY8, c.STACK_BINARY_F32) == (2, 3, 4) == (model.GRAY8, model.BINARY8, model.BINARY_F32)


def test_host_wrappers_reach_every_call():
    cs = re.sub(r"//.*", "", _read("gym.net_amd", "csharp", "VectorEnv.cs"))
    hpp = _read("include", "gymnet_amd.hpp")
    py = _read("gym.net_amd", "vector_env.py")
    for name in CALLS:
        assert "Native.%s(" % name in cs, name
        assert "%s(" % name in hpp, name
    for name in ("config", "reset_device", "push_device", "read"):
        assert "gymnet_vecenv_pixel_stack_%s(" % name in py, name
    for m in ("public void ConfigurePixelStack(", "public void ResetPixelStack(", "public void PushPixelStack(",
              "public void ReadPixelStack(Span<byte> destination", "public void ReadPixelStack(Span<float> destination"):
        assert m in cs, m
    for m in ("void ConfigurePixelStack(", "void ResetPixelStack(", "void PushPixelStack(", "std::vector<T> ReadPixelStack("):
        assert m in hpp, m


def test_python_api_has_the_stack_members(gymnet):
    assert callable(gymnet.VectorEnv.PixelStack)
    for m in ("Reset", "Push", "Step", "Read", "Close"):
        assert callable(getattr(gymnet.PixelFrameStack, m)), m


def test_calls_on_a_null_handle_are_refused(gymnet):
    lib = gymnet.load_library()
    buf = np.full(64, 0x5A, np.uint8)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    inv = gymnet._capi.ERR_INVALID_ARG
    assert lib.gymnet_vecenv_pixel_stack_config(None, 2, 2, *CROP, *SIZE, None, 0) == inv
    assert lib.gymnet_vecenv_pixel_stack_reset_device(None, None) == inv
    assert lib.gymnet_vecenv_pixel_stack_push_device(None, None) == inv
    assert lib.gymnet_vecenv_pixel_stack_view(None, None, None, None) == inv
    assert lib.gymnet_vecenv_pixel_stack_read(None, p, 0, 1) == inv
    assert (buf == 0x5A).all()


def test_model_hand_worked_sequence():
    def frames(*vals):                                     # lane k's 1 x 2 frame is [v, v + 1]
        return np.array([[[v, v + 1]] for v in vals], np.uint8)
    m = model.PixelStackModel(frames(10, 20, 30), 3)
    assert m.stack[:, :, 0, 0].tolist() == [[10, 10, 10], [20, 20, 20], [30, 30, 30]]
    m.push(frames(11, 21, 31))
    assert m.stack[:, :, 0, 0].tolist() == [[10, 10, 11], [20, 20, 21], [30, 30, 31]]
    m.push(frames(12, 22, 32), done=[0, 1, 0])            # lane 1 restarts: its frame in every slot
    assert m.stack[:, :, 0, 0].tolist() == [[10, 11, 12], [22, 22, 22], [30, 31, 32]]
    m.push(frames(13, 23, 33))
    assert m.stack[:, :, 0, 0].tolist() == [[11, 12, 13], [22, 22, 23], [31, 32, 33]]
    assert (m.stack[..., 1] == m.stack[..., 0] + 1).all()
    m.reset(frames(40, 50, 60), mask=[1, 0, 1])            # masked lanes only
    assert m.stack[:, :, 0, 0].tolist() == [[40, 40, 40], [22, 22, 23], [60, 60, 60]]
    m.reset(frames(41, 51, 61))
    assert m.stack[:, :, 0, 0].tolist() == [[41, 41, 41], [51, 51, 51], [61, 61, 61]]
    one = model.PixelStackModel(frames(1), 1)              # depth 1: the newest frame only
    one.push(frames(2))
    one.push(frames(3), done=[1])
    assert one.stack[:, :, 0, 0].tolist() == [[3]]


def test_model_formats():
    g = np.array([[[255, 254, 0, 160]]], np.uint8)
    assert model.process(g, model.GRAY8).tolist() == [[[255, 254, 0, 160]]]
    b = model.process(g, model.BINARY8)
    assert b.dtype == np.uint8 and b.tolist() == [[[0, 1, 1, 1]]]
    f = model.process(g, model.BINARY_F32)
    assert f.dtype == np.float32 and f.tolist() == [[[0.0, 1.0, 1.0, 1.0]]]


def test_model_on_twin_frames_in_the_images_runner_layout():
    """Known states drawn by the twin: an upright pole at the centre, then leaning right, then the cart moved left (a restart);
    the network input is 40 x 40 with the oldest frame on top and 1 where the pole or cart covers a sample."""
    def gray(x, th):
        f, amb = twin.render(x, th, twin.GRAY8, CROP, SIZE)
        return f[..., 0], amb
    g0, _ = gray([0.0, 0.0], [0.0, 0.0])
    g1, _ = gray([0.0, 0.1], [0.2, 0.0])
    g2, amb2 = gray([-0.5, 0.2], [0.0, 0.0])
    m = model.PixelStackModel(g0, 2, model.BINARY_F32)
    m.push(g1)
    net = m.network_input()
    assert net.shape == (2, 40, 40) and net.dtype == np.float32
    assert np.array_equal(net[:, :20], (g0 < 255).astype(np.float32)) and np.array_equal(net[:, 20:], (g1 < 255).astype(np.float32))
    # lane 0: the pole's upper part leans right in the newer (bottom) frame; the older shows it upright over columns 19..20
    top, bottom = net[0, :20], net[0, 20:]
    assert top[4:18, 19:21].all() and not top[:18, :19].any() and not top[:18, 21:].any()
    assert bottom[:4, 21:].any() and not np.array_equal(top, bottom)
    m.push(g2, done=[1, 0])
    net = m.network_input()
    assert np.array_equal(net[0, :20], net[0, 20:]) and np.array_equal(net[0, 20:], (g2[0] < 255).astype(np.float32))
    assert np.array_equal(net[1, :20], (g1[1] < 255).astype(np.float32)) and np.array_equal(net[1, 20:], (g2[1] < 255).astype(np.float32))
    # the cart at x = -0.5 (cx = 237.5) is left of the crop's centre: its pole covers columns 7..8 of the 40 (crop x 200, 5 px a column)
    assert amb2.sum() == 0 and net[0, 4:18, 7:9].all() and not net[0, :18, 10:].any()
