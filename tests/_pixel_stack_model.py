"""A NumPy restatement of the pixel frame stack contract (include/gymnet_amd.h, gymnet_vecenv_pixel_stack_config / _reset_device /
_push_device), fed with frames from elsewhere: GRAY8 frames the library rendered (gymnet_vecenv_render_device) or the twin's
(tests/_render_twin.py).

The stack is [N][depth][h][w], slot 0 the oldest.  reset(frames, mask) puts every masked lane's frame into all of its slots; push(frames,
done) puts a restarting lane's frame into all of its slots and shifts every other lane by one slot, the frame becoming the newest."""
import numpy as np

GRAY8, BINARY8, BINARY_F32 = 2, 3, 4


def process(gray, fmt):
    """A GRAY8 frame batch in the stack's element format: the gray values, 1 where gray < 255 as uint8, or that as float32."""
    gray = np.asarray(gray, np.uint8)
    if fmt == GRAY8:
        return gray.copy()
    binary = (gray < 255).astype(np.uint8)
    return binary if fmt == BINARY8 else binary.astype(np.float32)


class PixelStackModel:
    def __init__(self, gray, depth, fmt=GRAY8):
        """gray: uint8 [N, h, w], every lane's current frame; config fills every slot with it."""
        self.fmt, self.depth = fmt, int(depth)
        f = process(gray, fmt)
        self.stack = np.repeat(f[:, None], self.depth, axis=1)

    def reset(self, gray, mask=None):
        f = process(gray, self.fmt)
        sel = np.ones(len(f), bool) if mask is None else np.asarray(mask) != 0
        self.stack[sel] = f[sel, None]
        return self.stack

    def push(self, gray, done=None):
        f = process(gray, self.fmt)
        restart = np.zeros(len(f), bool) if done is None else np.asarray(done) != 0
        keep = ~restart
        self.stack[keep, :-1] = self.stack[keep, 1:]
        self.stack[keep, -1] = f[keep]
        self.stack[restart] = f[restart, None]
        return self.stack

    def network_input(self):
        """The Images runner's layout of one lane: the slots stacked vertically, the oldest on top ([N, depth * h, w])."""
        n, d, h, w = self.stack.shape
        return self.stack.reshape(n, d * h, w)
