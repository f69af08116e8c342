"""The numpy statement of the x4 chroma filter (cdfo_chroma_up4, include/cdfo_hip.h), written out for the tests: nothing here comes
from the package.  Output index j = 4q + r takes four taps from q-2 (r = 0, 1) or q-1 (r = 2, 3), indices clamped to the plane,
coefficients out of 128; x and y in integers without intermediate rounding; clamp((v + 8192) >> 14, 0, 255)."""
import numpy as np

COEF = np.array([[-6, 50, 93, -9], [-1, 12, 123, -6], [-6, 123, 12, -1], [-9, 93, 50, -6]], dtype=np.int64)


def up4_axis(a, axis):
    """int64 array -> four times as long along `axis`, scaled by 128."""
    a = np.moveaxis(np.asarray(a, dtype=np.int64), axis, -1)
    n = a.shape[-1]
    out = np.zeros(a.shape[:-1] + (4 * n,), dtype=np.int64)
    q = np.arange(n)
    for r in range(4):
        first = q - 2 if r < 2 else q - 1
        for k in range(4):
            out[..., r::4] += COEF[r, k] * a[..., np.clip(first + k, 0, n - 1)]
    return np.moveaxis(out, -1, axis)


def up4_sums(p, x_first=True):
    """The integer sums before the final shift, [..., 4h, 4w], scaled by 128 * 128."""
    return up4_axis(up4_axis(p, -1), -2) if x_first else up4_axis(up4_axis(p, -2), -1)


def up4(p, x_first=True):
    """uint8 [..., h, w] -> uint8 [..., 4h, 4w]; `>>` on negative int64 is an arithmetic shift, i.e. a floor."""
    return np.ascontiguousarray(np.clip((up4_sums(p, x_first) + 8192) >> 14, 0, 255).astype(np.uint8))


def catmull_rom_float(p):
    """float64 Catmull-Rom sampled at (j + 0.5) / 4 - 0.5 along both axes with edge replication, rounded and clipped."""
    def axis(a, ax):
        a = np.moveaxis(np.asarray(a, dtype=np.float64), ax, -1)
        n = a.shape[-1]
        s = (np.arange(4 * n) + 0.5) / 4.0 - 0.5
        i = np.floor(s).astype(np.int64)
        t = s - i
        w = [(-t ** 3 + 2 * t ** 2 - t) / 2, (3 * t ** 3 - 5 * t ** 2 + 2) / 2, (-3 * t ** 3 + 4 * t ** 2 + t) / 2, (t ** 3 - t ** 2) / 2]
        out = sum(w[k] * a[..., np.clip(i - 1 + k, 0, n - 1)] for k in range(4))
        return np.moveaxis(out, -1, ax)
    return np.clip(np.rint(axis(axis(p, -1), -2)), 0, 255)


def contents(shape, seed):
    """The three kinds of plane the tests use: random bytes, a 0/255 checkerboard, random 0/255 (the last two drive the sums below 0
    and above 255)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.indices(shape[-2:])
    board = np.broadcast_to((((yy + xx) % 2) * 255).astype(np.uint8), shape).copy()
    return dict(random=rs.randint(0, 256, shape).astype(np.uint8), checkerboard=board,
                binary=(rs.randint(0, 2, shape) * 255).astype(np.uint8))
