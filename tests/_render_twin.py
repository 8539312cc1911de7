"""An independent NumPy restatement of the CartPole frame contract (include/gymnet_amd.h, gymnet_vecenv_render_device), in float64.

The canvas is CartPoleEnv.Render's (CartPoleEnv.cs:69-135): 600 x 400, y down, shapes painted in order (last wins) — background white,
track black [0, 600) x [300, 301), cart black [cx - 25, cx + 25] x [285, 315], pole (204, 153, 102) = u in [-5, 5], v in [5 - polelen, 5]
about the pivot (cx, 295) with u = dx cos t + dy sin t, v = dy cos t - dx sin t, axle (204, 153, 102) = the disc of radius 5 at the pivot.
Each output pixel is the rounded mean of a 4 x 4 grid of samples.

Besides the frame, render() returns per pixel how many of its samples lie within EPS canvas pixels of an edge of a shape: the kernel
decides those in float32 (its own sin / cos, its own sample positions) and may decide them either way.  Such a pixel is AMBIGUOUS and
may differ by at most ceil(255 * k / 16) per channel, k = its ambiguous samples."""
import numpy as np

WIDTH, HEIGHT = 600, 400
SCALE = np.float32(600.0) / (np.float32(2.4) * np.float32(2.0))       # the C# float constant 124.99999237f
POLE_LEN = SCALE * (np.float32(2.0) * np.float32(0.5))
PIVOT_Y = 295.0
EPS = 1e-3
RGB8, GRAY8 = 1, 2
WHITE, BLACK, POLE = 0, 1, 2
COLOURS = {RGB8: np.array([[255, 255, 255], [0, 0, 0], [204, 153, 102]], np.int64), GRAY8: np.array([[255], [0], [160]], np.int64)}


def cart_x(x):
    """(float)((double)x * scale + 300.0), element-wise; x float32 or float64."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(x, np.float64) * np.float64(SCALE) + 300.0).astype(np.float32)


def sample_positions(crop, size):
    cx0, cy0, cw, ch = crop
    w, h = size
    q = (np.arange(4) + 0.5) / 4.0
    xs = cx0 + (np.arange(w)[:, None] + q[None, :]).reshape(-1) * (cw / w)
    ys = cy0 + (np.arange(h)[:, None] + q[None, :]).reshape(-1) * (ch / h)
    return xs, ys                                                        # (4 w,), (4 h,): sample a of pixel j is xs[4 j + a]


def _paint(x, theta, xs, ys):
    """Paint index and ambiguity flag of every sample, for a batch of lanes: (L, 4h, 4w) each."""
    L = len(x)
    cx = cart_x(x).astype(np.float64)[:, None, None]
    t = np.asarray(theta, np.float32).astype(np.float64)[:, None, None]
    X = xs[None, None, :]
    Y = ys[None, :, None]
    paint = np.zeros((L, len(ys), len(xs)), np.int8)
    amb = np.zeros(paint.shape, bool)
    track = (Y >= 300.0) & (Y < 301.0)
    paint[np.broadcast_to(track, paint.shape)] = BLACK
    amb |= np.broadcast_to((np.abs(Y - 300.0) < EPS) | (np.abs(Y - 301.0) < EPS), paint.shape)
    fx = np.isfinite(cx)
    ft = fx & np.isfinite(t)
    with np.errstate(invalid="ignore", over="ignore"):
        cxs = np.where(fx, cx, 0.0)
        dx = X - cxs
        dy = Y - PIVOT_Y
        # cart
        cl, cr = cxs - 25.0, cxs + 25.0
        inside = fx & (X >= cl) & (X <= cr) & (Y >= 285.0) & (Y <= 315.0)
        paint[inside] = BLACK
        near = ((np.minimum(np.abs(X - cl), np.abs(X - cr)) < EPS) & (Y >= 285.0 - EPS) & (Y <= 315.0 + EPS)) | \
               ((np.minimum(np.abs(Y - 285.0), np.abs(Y - 315.0)) < EPS) & (X >= cl - EPS) & (X <= cr + EPS))
        amb |= fx & near
        # pole
        tt = np.where(ft, t, 0.0)
        c, s = np.cos(tt), np.sin(tt)
        u = dx * c + dy * s
        v = dy * c - dx * s
        vlo = 5.0 - np.float64(POLE_LEN)
        inside = ft & (np.abs(u) <= 5.0) & (v >= vlo) & (v <= 5.0)
        paint[inside] = POLE
        near = ((np.abs(np.abs(u) - 5.0) < EPS) & (v >= vlo - EPS) & (v <= 5.0 + EPS)) | \
               ((np.minimum(np.abs(v - vlo), np.abs(v - 5.0)) < EPS) & (np.abs(u) <= 5.0 + EPS))
        amb |= ft & near
        # axle
        r = np.sqrt(dx * dx + dy * dy)
        paint[fx & (r <= 5.0)] = POLE
        amb |= fx & (np.abs(r - 5.0) < EPS)
    return paint, amb


def render(x, theta, fmt=RGB8, crop=(0, 0, WIDTH, HEIGHT), size=None):
    """Frames of lanes with cart position x[k] and pole angle theta[k]: (uint8 [L, h, w, C], ambiguous-sample counts int [L, h, w])."""
    x = np.atleast_1d(x)
    theta = np.atleast_1d(theta)
    w, h = (crop[2], crop[3]) if size is None else size
    xs, ys = sample_positions(crop, (w, h))
    col = COLOURS[fmt]
    batch = max(1, (1 << 21) // (len(xs) * len(ys)))                    # lanes per pass: a few hundred MB of temporaries at most
    frames = np.empty((len(x), h, w, col.shape[1]), np.uint8)
    amb_count = np.empty((len(x), h, w), np.int64)
    for b in range(0, len(x), batch):
        paint, amb = _paint(x[b:b + batch], theta[b:b + batch], xs, ys)
        n = paint.shape[0]
        vals = col[paint]                                                     # (n, 4h, 4w, C)
        sums = vals.reshape(n, h, 4, w, 4, -1).sum(axis=(2, 4))
        frames[b:b + batch] = (sums + 8) >> 4
        amb_count[b:b + batch] = amb.reshape(n, h, 4, w, 4).sum(axis=(2, 4))
    return frames, amb_count


def compare(got, want, amb_count):
    """Checks a kernel frame batch against the twin: unambiguous pixels exactly, ambiguous ones within ceil(255 k / 16) per channel.
    Returns the fraction of pixels that are ambiguous."""
    got = np.asarray(got, np.int64).reshape(want.shape)
    diff = np.abs(got - want.astype(np.int64)).max(axis=-1)
    bound = -(-255 * amb_count // 16)
    bad = diff > bound
    assert not bad.any(), f"{int(bad.sum())} pixels off (first at {np.argwhere(bad)[0].tolist()}: got " \
                          f"{got[tuple(np.argwhere(bad)[0])]}, want {want[tuple(np.argwhere(bad)[0])]}, ambiguous samples " \
                          f"{amb_count[tuple(np.argwhere(bad)[0])]})"
    return float((amb_count > 0).mean())
