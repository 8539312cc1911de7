"""CPU checks of CartPole rendering (gymnet_vecenv_render / _render_device): the library exports both calls, every binding declares
them, the header carries the format values, and the NumPy twin the GPU tests compare against draws the reference's geometry
(CartPoleEnv.cs:69-135) at known states."""
import ctypes
import os
import re

import numpy as np

import _render_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("gymnet_vecenv_render_device", "gymnet_vecenv_render")
POLE = [204, 153, 102]


def test_library_and_bindings_declare_the_render_calls(gymnet):
    lib = ctypes.CDLL(gymnet.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gymnet_amd.h")).read()
    native = open(os.path.join(ROOT, "gym.net_amd", "csharp", "Native.cs")).read()
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in gymnet._capi.PROTOTYPES and len(gymnet._capi.PROTOTYPES[name][1]) == 12
        assert re.search(r"\[DllImport\(Lib\)\] public static extern int %s\(" % name, native), name
    assert "enum { GYMNET_PIXELS_RGB8 = 1, GYMNET_PIXELS_GRAY8 = 2 };" in hdr
    assert (gymnet._capi.PIXELS_RGB8, gymnet._capi.PIXELS_GRAY8) == (1, 2) == (twin.RGB8, twin.GRAY8)
    assert "public enum GymnetPixelFormat { Rgb8 = 1, Gray8 = 2 }" in native
    # the single-instance facades and the C# VectorEnv reach the host call
    for f in ("GpuEnv.cs", "VectorEnv.cs"):
        assert "Native.gymnet_vecenv_render(" in open(os.path.join(ROOT, "gym.net_amd", "csharp", f)).read(), f


def test_python_api_has_the_render_members(gymnet):
    for m in ("Render", "RenderDevice", "RenderFrames"):
        assert callable(getattr(gymnet.VectorEnv, m)), m
    assert callable(gymnet.GpuEnv.Render)


def test_twin_constants_are_the_csharp_floats():
    assert twin.SCALE == np.float32(124.99999237060547) and twin.SCALE != np.float32(125.0)
    assert twin.POLE_LEN == twin.SCALE
    assert twin.cart_x(np.float32(0.0)) == np.float32(300.0)
    assert twin.cart_x(np.float64(1.2)) == np.float32(1.2 * np.float64(twin.SCALE) + 300.0)


def test_twin_upright_pole_at_the_centre():
    f, amb = twin.render([0.0], [0.0])
    f = f[0]
    assert f.shape == (400, 600, 3) and f.dtype == np.uint8 and amb.sum() == 0
    is_pole = (f == POLE).all(-1)
    is_black = (f == 0).all(-1)
    # the track row is black across the canvas; the rows around it are white away from the cart
    assert is_black[300].all()
    assert (f[299, :270] == 255).all() and (f[301, :270] == 255).all() and (f[299, 330:] == 255).all()
    # the cart: [275, 325] x [285, 315], black where neither pole nor axle covers it
    assert is_black[286:315, 276:325][~is_pole[286:315, 276:325]].all()
    assert (f[285, 276:325] != 255).all() and (f[314, 276:325] == 0).all()
    assert (f[310, 274] == 255).all() and (f[310, 325] == 255).all() and (f[310, 275] == 0).all() and (f[310, 324] == 0).all()
    # the pole: rows 175..299 over columns 295..304, nothing of it above row 175
    cols = np.where(is_pole.any(0))[0]
    rows = np.where(is_pole.any(1))[0]
    assert (cols.min(), cols.max()) == (295, 304) and (rows.min(), rows.max()) == (175, 299)
    assert is_pole[175:285, 295:305].all() and not is_pole[:175].any()
    # the axle disc (radius 5) lies inside the pole's pivot end whenever the pole is drawn: with a non-finite angle it shows alone,
    # centred at (300, 295) inside the black cart
    g, amb = twin.render([0.0], [np.nan])
    disc = (g[0] == POLE).all(-1)
    ys, xs = np.nonzero(disc)
    assert amb.sum() == 0 and 60 <= disc.sum() <= 80
    assert (xs.mean() + 0.5, ys.mean() + 0.5) == (300.0, 295.0)
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (295, 304, 290, 299)


def test_twin_positive_theta_leans_the_pole_right_and_x_moves_the_cart():
    f0, _ = twin.render([0.0], [0.0])
    f1, _ = twin.render([0.0], [0.2])
    tip0 = np.where((f0[0, 180] == POLE).all(-1))[0]
    tip1 = np.where((f1[0, 180] == POLE).all(-1))[0]
    assert tip1.min() > tip0.max()                         # the tip moves right
    assert tip1.mean() - 300 > 20                          # ~ 115 px * sin(0.2)
    f2, _ = twin.render([-1.2], [0.0])                     # cx = 300 - 150 = 150
    cols = np.where((f2[0, 310] == 0).all(-1))[0]
    assert (cols.min(), cols.max()) == (125, 174)


def test_twin_gray_crop_and_non_finite_lanes():
    g, amb = twin.render([0.0, np.nan, 0.0], [0.0, 0.0, np.inf], twin.GRAY8, (200, 150, 200, 150), (40, 20))
    assert g.shape == (3, 20, 40, 1) and amb.sum() == 0
    assert set(np.unique(g[0])) >= {0, 160, 255}
    # a non-finite x: background and track only (the track row y = 300 lies below this crop); a non-finite angle: no pole, the
    # cart and the axle stay
    assert (g[1] == 255).all()
    assert (g[0][4:18, 19:21] == 160).all() and not (g[2][:18] == 160).any()
    assert (g[2][18, 15:18] == 0).all() and (g[2][18:, 19:21] > 0).all()
