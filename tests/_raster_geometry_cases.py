"""The case table of the frame kernels' geometry tests (tests/test_raster_geometry_host.py, tests/test_gpu_raster_geometry.py): output
geometries and lane states at which render_kernel, pixel_stack_kernel and memory_frames_kernel (one rasteriser,
gym.net_amd/csrc/cartpole_raster.hpp, one work decomposition: a wave covers 1024 consecutive pixels of one frame, 16 per thread) are
held to the float64 twin (tests/_render_twin.py), and a copy of the twin's painter with deliberate mistakes that proves each case
would notice one.

truth(name, dtype) is the twin's answer for a case's state set, computed once per process and shared by every test that needs it."""
import functools

import numpy as np

import _render_twin as twin

CANVAS = (0, 0, 600, 400)
BIG = 50_000                       # pixels per frame above which a case uses the first SUBSET lanes only (the twin costs seconds per lane)
SUBSET = 24
AMBIGUOUS_CAP = 0.002              # share of pixels, over all lanes of a case, that may hold a sample within twin.EPS of an edge

# mistakes of mistaken_gray(); a case lists the ones that cannot show in it, and why
OFFSET, ORIGIN, SWAP, POLE_SHIFT, BBOX = "sample offset 0.0", "crop origin + 1", "sxq / syq swapped", "pole v-range + 1", "bounding box - 6"
MISTAKES = (OFFSET, ORIGIN, SWAP, POLE_SHIFT, BBOX)
_SQUARE = {SWAP: "crop_w / out_w == crop_h / out_h: swapping the two steps changes nothing"}
_BACKGROUND = {m: "the crop shows nothing but background under every state: no shape, no edge, nothing to move" for m in MISTAKES}

# name: (crop, size, the paths of the kernels it reaches, {mistake: why it cannot show})
CASES = {
    "1x1": (CANVAS, (1, 1), "a frame of 1 byte (GRAY8, BINARY8), 3 bytes (RGB8) or one dword (BINARY_F32): nb < 16 C, byte / dword tail only", {}),
    "5x3": (CANVAS, (5, 3), "15 pixels: shorter than one thread's 16, the row wraps three times inside it; odd frame_bytes", {}),
    "1x37": (CANVAS, (1, 37), "out_w = 1: the row wraps after every pixel; 37 bytes", {}),
    "17x61": (CANVAS, (17, 61), "1037 pixels: the second wave holds 13 (ragged last wave, one thread with a tail); odd frame_bytes, so packed frames "
              "alternate between the dwordx4 path and the byte path; RGB8 away from 600 x 400", {}),
    "84x84": ((200, 150, 200, 150), (84, 84), "non-integer ratios 2.38 / 1.79 under a crop; 6.9 waves", {}),
    "up4": ((270, 240, 64, 80), (256, 320), "4 x upscale (sxq = syq = 1 / 16), 80 waves", _SQUARE),
    "up32": ((299, 294, 2, 2), (64, 64), "32 x upscale on the axle (sxq = 1 / 128)", _SQUARE),
    "wide": ((0, 299, 600, 2), (16384, 1), "the width limit kRenderMaxSide: sample index 4 j + a up to 65535", {}),
    "tall": ((299, 0, 2, 400), (1, 16384), "the height limit with out_w = 1", {}),
    "background": ((0, 0, 50, 50), (10, 10), "nothing but background: every sample row misses the bounding box", _BACKGROUND),
    "edge": ((550, 290, 50, 20), (25, 10), "the canvas edge, the cart partly inside; 250 pixels", _SQUARE),
    "odd": ((37, 101, 501, 263), (97, 53), "odd everything: 5141 pixels, ratios 5.16 / 4.96", {}),
    "160x210": (CANVAS, (160, 210), "x down by 3.75, y down by 1.90; 33600 pixels", {}),
}
NAMES = tuple(CASES)
SMALL = tuple(k for k in NAMES if CASES[k][1][0] * CASES[k][1][1] <= BIG)


def crop_size(name):
    return CASES[name][0], CASES[name][1]


def pixels(name):
    w, h = CASES[name][1]
    return w * h


def waves(name):
    """Waves per frame: 1024 pixels each."""
    return (pixels(name) + 1023) // 1024


def edge_rows():
    """The 56 rows of _edge_states in tests/test_gpu_render.py, as (x, theta): the 49 finite ones, then the 7 that are not."""
    xs = [0.0, 1.2, -1.2, 2.4, -2.4, 3.0, -3.0]
    ths = [0.0, 0.2, -0.2, np.pi / 2, -np.pi / 2, np.pi, 7.0]
    finite = [(x, t) for x in xs for t in ths]
    rest = [(np.nan, 0.0), (np.inf, 0.1), (-np.inf, 0.0), (0.5, np.nan), (-0.5, np.inf), (0.0, -np.inf), (np.nan, np.nan)]
    return finite, rest


def _rows(dtype):
    finite, rest = edge_rows()
    f32max = float(np.finfo(np.float32).max)
    # theta beyond 65536 (sincos_f32 leaves its own reduction for the device library) and a large one inside it; a cart that is finite
    # but far off the canvas; one whose cx overflows float32; signed zeros; float32 subnormals
    extra = [(0.3, 7.0e4), (-0.3, -1.0e4), (1e30, 0.1), (f32max, 0.1), (-0.0, -0.0), (1e-40, 1e-40)]
    if np.dtype(dtype) == np.float64:
        extra.append((1e300, 1e300))
    # lanes aimed at the two cases whose window is too narrow for the states above to put an edge into it.  "1x1": the pole's tip half
    # a pixel inside sample (225, 250) of the whole canvas (its 16 samples are 150 x 100 px apart).  "up32" (2 x 2 px about (300, 295)):
    # a horizontal pole whose pivot end (v = 5) and axle rim cross the window, and a cart whose left edge is 3 px from it, so that
    # the window lies in the margin of the bounding box
    aimed = [(0.2856, -1.1847), (0.044, np.pi / 2), (0.176, 0.0)]
    rng = np.random.default_rng(0xC0FFEE)
    rnd = list(zip(rng.uniform(-2.6, 2.6, 40), rng.uniform(-np.pi, np.pi, 40)))
    # the first SUBSET lanes are what a case above BIG pixels uses: every non-finite row, the additions and the first finite edge rows
    return rest + extra + aimed + finite + rnd


def states(dtype, name=None):
    """State rows [4, L] of dtype for a case (None: the full set): x in row 0, theta in row 2."""
    rows = _rows(dtype)
    if name is not None and pixels(name) > BIG:
        rows = rows[:SUBSET]
    s = np.zeros((4, len(rows)), dtype)
    with np.errstate(over="ignore"):
        s[0] = np.array([r[0] for r in rows], np.float64).astype(dtype)
        s[2] = np.array([r[1] for r in rows], np.float64).astype(dtype)
    s[1], s[3] = 0.3, -0.7
    return s


def _reduce(paint, fmt, h, w):
    n = paint.shape[0]
    sums = twin.COLOURS[fmt][paint].reshape(n, h, 4, w, 4, -1).sum(axis=(2, 4))
    return ((sums + 8) >> 4).astype(np.uint8)


def frames_of(x, theta, crop, size):
    """twin.render's frames in both formats from ONE painting: (rgb uint8 [L, h, w, 3], gray uint8 [L, h, w, 1], ambiguous-sample
    counts int64 [L, h, w]).  test_raster_geometry_host.py checks it against twin.render itself."""
    x, theta = np.atleast_1d(x), np.atleast_1d(theta)
    w, h = size
    xs, ys = twin.sample_positions(crop, size)
    batch = max(1, (1 << 21) // (len(xs) * len(ys)))
    rgb = np.empty((len(x), h, w, 3), np.uint8)
    gray = np.empty((len(x), h, w, 1), np.uint8)
    amb = np.empty((len(x), h, w), np.int64)
    for b in range(0, len(x), batch):
        paint, near = twin._paint(x[b:b + batch], theta[b:b + batch], xs, ys)
        rgb[b:b + batch] = _reduce(paint, twin.RGB8, h, w)
        gray[b:b + batch] = _reduce(paint, twin.GRAY8, h, w)
        amb[b:b + batch] = near.reshape(paint.shape[0], h, 4, w, 4).sum(axis=(2, 4))
    return rgb, gray, amb


@functools.lru_cache(maxsize=None)
def truth(name, dtype):
    """The twin's frames of states(dtype, name) at case `name`: {twin.RGB8: frames, twin.GRAY8: frames, "amb": counts}.  Read-only."""
    s = states(dtype, name)
    rgb, gray, amb = frames_of(s[0], s[2], *crop_size(name))
    for a in (rgb, gray, amb):
        a.setflags(write=False)
    return {twin.RGB8: rgb, twin.GRAY8: gray, "amb": amb}


def mistaken_gray(x, theta, crop, size, mistake):
    """GRAY8 frames [L, h, w, 1] of a painter that restates twin._paint (the same shapes in the same order) with ONE deliberate mistake
    of the kind a rewrite of cartpole_raster.hpp could make; mistake=None paints what the twin paints."""
    assert mistake is None or mistake in MISTAKES
    cx0, cy0, cw, ch = crop
    w, h = size
    if mistake == ORIGIN:
        cx0, cy0 = cx0 + 1, cy0 + 1
    q = (np.arange(4) + (0.0 if mistake == OFFSET else 0.5)) / 4.0
    stepx, stepy = (ch / h, cw / w) if mistake == SWAP else (cw / w, ch / h)
    X = (cx0 + (np.arange(w)[:, None] + q[None, :]).reshape(-1) * stepx)[None, None, :]
    Y = (cy0 + (np.arange(h)[:, None] + q[None, :]).reshape(-1) * stepy)[None, :, None]
    x, theta = np.atleast_1d(x), np.atleast_1d(theta)
    cx = twin.cart_x(x).astype(np.float64)[:, None, None]
    with np.errstate(over="ignore"):
        t = np.asarray(theta, np.float32).astype(np.float64)[:, None, None]
    paint = np.zeros((len(x), 4 * h, 4 * w), np.int8)
    track = np.broadcast_to((Y >= 300.0) & (Y < 301.0), paint.shape)
    paint[track] = twin.BLACK
    fx = np.isfinite(cx)
    ft = fx & np.isfinite(t)
    with np.errstate(invalid="ignore", over="ignore"):
        cxs = np.where(fx, cx, 0.0)
        dx, dy = X - cxs, Y - twin.PIVOT_Y
        cart = fx & (np.abs(dx) <= 25.0) & (Y >= 285.0) & (Y <= 315.0)
        c, s = np.cos(np.where(ft, t, 0.0)), np.sin(np.where(ft, t, 0.0))
        u, v = dx * c + dy * s, dy * c - dx * s
        vlo, vhi = 5.0 - np.float64(twin.POLE_LEN), 5.0
        if mistake == POLE_SHIFT:
            vlo, vhi = vlo + 1.0, vhi + 1.0
        pole = ft & (np.abs(u) <= 5.0) & (v >= vlo) & (v <= vhi)
        axle = fx & (dx * dx + dy * dy <= 25.0)
        if mistake == BBOX:
            # the kernel's cull, too tight: samples outside the box of cart + pole corners, shrunk by 6 px a side, see background and track
            lo_x, hi_x, lo_y, hi_y = np.full_like(cx, -25.0), np.full_like(cx, 25.0), np.full_like(cx, -10.0), np.full_like(cx, 20.0)
            for cu in (-5.0, 5.0):
                for cv in (5.0 - np.float64(twin.POLE_LEN), 5.0):
                    px, py = np.where(ft, cu * c - cv * s, 0.0), np.where(ft, cu * s + cv * c, 0.0)
                    lo_x, hi_x, lo_y, hi_y = np.minimum(lo_x, px), np.maximum(hi_x, px), np.minimum(lo_y, py), np.maximum(hi_y, py)
            box = (dx >= lo_x + 6.0) & (dx <= hi_x - 6.0) & (dy >= lo_y + 6.0) & (dy <= hi_y - 6.0)
            cart, pole, axle = cart & box, pole & box, axle & box
        paint[cart] = twin.BLACK
        paint[pole] = twin.POLE
        paint[axle] = twin.POLE
    return _reduce(paint, twin.GRAY8, h, w)
