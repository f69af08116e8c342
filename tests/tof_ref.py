"""ORACLE (test infrastructure only): the fp64 numpy statement of the project's tOF, stage by stage.

tOF of frame t is the mean endpoint distance between the dense Farneback flow of (gt[t-1], gt[t]) and that of (sr[t-1], sr[t]) over
the whole common region of the 8-bit luma frames, with the reference's arguments (pyr_scale 0.5, levels 3, winsize 15, iterations 3,
poly_n 5, poly_sigma 1.2, flags 0).  The definition is the project's own, written after the algorithm OpenCV documents; cv2 is not
available to pin it against.  Every sum below has a fixed order (taps in index order, accumulator starting at 0.0) and no product is
contracted with the add behind it, so the device kernels can follow it term by term.

Stages (the names the tests address): `levels` (the stage sizes), `level_image` (smooth + resize of one frame), `polyexp` (the five
coefficient planes), `matrices` (the five planes of the normal equations from both expansions and a flow), `blur_solve` (15 x 15 box
mean, 2 x 2 solve), `flow_up` (a flow onto the next stage's grid, times 2), `farneback` (all of them), `tof`."""
import numpy as np

MIN_SIZE = 32
LEVELS, WINSIZE, ITERATIONS, POLY_N, POLY_SIGMA = 3, 15, 3, 5, 1.2
BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)


def levels(H: int, W: int):
    """[(k, h, w)] for the stages k = L .. 0 of an H x W frame; ValueError below 32 x 32."""
    H, W = int(H), int(W)
    if H < MIN_SIZE or W < MIN_SIZE:
        raise ValueError(f"tOF needs frames of at least {MIN_SIZE} x {MIN_SIZE}, got {H} x {W}")
    L, s = 0, 1.0
    for k in range(LEVELS):
        s *= 0.5
        if W * s < MIN_SIZE or H * s < MIN_SIZE:
            break
        L = k + 1
    return [(k, int(np.rint(H * 0.5 ** k)), int(np.rint(W * 0.5 ** k))) for k in range(L, -1, -1)]


def smooth_taps(k: int) -> np.ndarray:
    """The taps of stage k's smoothing: sigma = (2^k - 1) / 2, n = max(rint(5 sigma) | 1, 3) taps exp(-x^2 / 2 sigma^2) normalised;
    [1/4, 1/2, 1/4] at sigma = 0."""
    sigma = (1.0 / 0.5 ** k - 1.0) / 2.0
    n = max(int(np.rint(5.0 * sigma)) | 1, 3)
    if sigma == 0.0:
        return np.array([0.25, 0.5, 0.25])
    x = np.arange(n, dtype=np.float64) - (n - 1) // 2
    t = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return t / t.sum()


def _reflect101(i: np.ndarray, n: int) -> np.ndarray:
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def _taps_along(img: np.ndarray, taps: np.ndarray, axis: int, index) -> np.ndarray:
    """sum_j taps[j] img[index(i + j - r)] along ``axis``, j ascending from an accumulator of 0.0."""
    n, r = img.shape[axis], (len(taps) - 1) // 2
    at = np.arange(n)
    acc = np.zeros_like(img)
    for j, t in enumerate(taps):
        acc = acc + t * np.take(img, index(at + j - r, n), axis=axis)
    return acc


def _resize_axis(N: int, n: int):
    """(i0, i1, weight) of the bilinear resize of N samples to n: the source coordinate (i + 1/2) (N / n) - 1/2, the two taps clamped
    into the image, the weight from the unclamped floor."""
    f = (np.arange(n, dtype=np.float64) + 0.5) * (float(N) / float(n)) - 0.5
    i0 = np.floor(f)
    wgt = f - i0
    i0 = i0.astype(np.int64)
    return np.clip(i0, 0, N - 1), np.clip(i0 + 1, 0, N - 1), wgt


def resize(img: np.ndarray, h: int, w: int) -> np.ndarray:
    """[H,W,...] -> [h,w,...] bilinearly: along x on both rows, then along y; (1 - a) p + a q each time."""
    H, W = img.shape[:2]
    y0, y1, wy = _resize_axis(H, h)
    x0, x1, wx = _resize_axis(W, w)
    wy = wy.reshape((h, 1) + (1,) * (img.ndim - 2))
    wx = wx.reshape((1, w) + (1,) * (img.ndim - 2))
    top = (1.0 - wx) * img[y0][:, x0] + wx * img[y0][:, x1]
    bot = (1.0 - wx) * img[y1][:, x0] + wx * img[y1][:, x1]
    return (1.0 - wy) * top + wy * bot


def level_image(frame: np.ndarray, k: int, h: int, w: int) -> np.ndarray:
    """uint8 [H,W] -> fp64 [h,w]: stage k's smoothing down the columns, then along the rows, reflect-101; then the resize."""
    x = frame.astype(np.float64)
    taps = smooth_taps(k)
    x = _taps_along(x, taps, 0, _reflect101)
    x = _taps_along(x, taps, 1, _reflect101)
    return resize(x, h, w)


def flow_up(flow: np.ndarray, h: int, w: int) -> np.ndarray:
    """fp64 [hp,wp,2] -> [h,w,2]: the previous stage's flow on this stage's grid, times 2."""
    return 2.0 * resize(flow, h, w)


def poly_kernels():
    """(g, xg, xxg, ig11, ig03, ig33, ig55): the 11 taps of each kind and the four entries of the inverse Gram matrix of the basis
    1, x, y, x^2, y^2, xy under g (x) g that are not zero by symmetry."""
    x = np.arange(-POLY_N, POLY_N + 1, dtype=np.float64)
    g = np.exp(-(x * x) / (2.0 * POLY_SIGMA * POLY_SIGMA))
    g = g / g.sum()
    xg = x * g
    xxg = x * x * g
    X, Y = np.meshgrid(x, x)
    basis = np.stack([np.ones_like(X), X, Y, X * X, Y * Y, X * Y]).reshape(6, -1)
    G = (basis * np.outer(g, g).reshape(-1)) @ basis.T
    inv = np.linalg.inv(G)
    return g, xg, xxg, inv[1, 1], inv[0, 3], inv[3, 3], inv[5, 5]


def _clamp(i: np.ndarray, n: int) -> np.ndarray:
    return np.clip(i, 0, n - 1)


def polyexp(img: np.ndarray) -> np.ndarray:
    """fp64 [h,w] -> [5,h,w] = (b_x, b_y, a_xx, a_yy, a_xy): the six separable moments (columns first, then rows, the edge sample
    repeated) times the inverse Gram matrix."""
    g, xg, xxg, ig11, ig03, ig33, ig55 = poly_kernels()
    v0, v1, v2 = (_taps_along(img, t, 0, _clamp) for t in (g, xg, xxg))
    m0, m1, m3 = (_taps_along(v0, t, 1, _clamp) for t in (g, xg, xxg))
    m2, m5 = (_taps_along(v1, t, 1, _clamp) for t in (g, xg))
    m4 = _taps_along(v2, g, 1, _clamp)
    return np.stack([m1 * ig11, m2 * ig11, m0 * ig03 + m3 * ig33, m0 * ig03 + m4 * ig33, m5 * ig55])


def border_scale(h: int, w: int) -> np.ndarray:
    """fp64 [h,w]: the product, from 1.0, of the left, right, top and bottom factors in that order."""
    b = np.array(BORDER)
    s = np.ones((h, w))
    x, y = np.arange(w), np.arange(h)
    s = s * np.where(x < 5, b[np.minimum(x, 4)], 1.0)[None, :]
    s = s * np.where(x >= w - 5, b[np.minimum(w - 1 - x, 4)], 1.0)[None, :]
    s = s * np.where(y < 5, b[np.minimum(y, 4)], 1.0)[:, None]
    s = s * np.where(y >= h - 5, b[np.minimum(h - 1 - y, 4)], 1.0)[:, None]
    return s


def matrices(R0: np.ndarray, R1: np.ndarray, flow: np.ndarray) -> np.ndarray:
    """R0, R1 fp64 [5,h,w], flow [h,w,2] (dx, dy) -> M fp64 [5,h,w]."""
    _, h, w = R0.shape
    dx, dy = flow[..., 0], flow[..., 1]
    fx = np.arange(w, dtype=np.float64)[None, :] + dx
    fy = np.arange(h, dtype=np.float64)[:, None] + dy
    inside = (fx >= 0.0) & (fx < w - 1) & (fy >= 0.0) & (fy < h - 1)
    x1 = np.where(inside, np.floor(fx), 0.0).astype(np.int64)
    y1 = np.where(inside, np.floor(fy), 0.0).astype(np.int64)
    a0, a1 = fx - x1, fy - y1
    w00, w01, w10, w11 = (1.0 - a1) * (1.0 - a0), (1.0 - a1) * a0, a1 * (1.0 - a0), a1 * a0
    x2, y2 = np.minimum(x1 + 1, w - 1), np.minimum(y1 + 1, h - 1)          # only read where inside
    S = w00 * R1[:, y1, x1] + w01 * R1[:, y1, x2] + w10 * R1[:, y2, x1] + w11 * R1[:, y2, x2]
    axx = np.where(inside, (R0[2] + S[2]) * 0.5, R0[2])
    ayy = np.where(inside, (R0[3] + S[3]) * 0.5, R0[3])
    axy = np.where(inside, (R0[4] + S[4]) * 0.25, R0[4] * 0.5)
    b1x, b1y = np.where(inside, S[0], 0.0), np.where(inside, S[1], 0.0)
    bx = (R0[0] - b1x) * 0.5 + axx * dx + axy * dy
    by = (R0[1] - b1y) * 0.5 + axy * dx + ayy * dy
    s = border_scale(h, w)
    axx, ayy, axy, bx, by = axx * s, ayy * s, axy * s, bx * s, by * s
    return np.stack([axx * axx + axy * axy, (axx + ayy) * axy, ayy * ayy + axy * axy, axx * bx + axy * by, axy * bx + ayy * by])


def box_mean(M: np.ndarray) -> np.ndarray:
    """[...,h,w]: the 15 x 15 box mean, the edge sample repeated: 15 rows added top to bottom, 15 of those sums added left to right,
    divided by 225."""
    ones = np.ones(WINSIZE)
    v = _taps_along(M, ones, M.ndim - 2, _clamp)
    return _taps_along(v, ones, M.ndim - 1, _clamp) / float(WINSIZE * WINSIZE)


def blur_solve(M: np.ndarray) -> np.ndarray:
    """M fp64 [5,h,w] -> flow [h,w,2]."""
    g11, g12, g22, h1, h2 = box_mean(M)
    idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3)
    return np.stack([(g22 * h1 - g12 * h2) * idet, (g11 * h2 - g12 * h1) * idet], axis=-1)


def farneback(prev: np.ndarray, cur: np.ndarray) -> np.ndarray:
    """uint8 [H,W] twice -> the flow fp64 [H,W,2] from ``prev`` to ``cur``."""
    if prev.shape != cur.shape or prev.ndim != 2:
        raise ValueError(f"two frames of one size expected, got {prev.shape} and {cur.shape}")
    flow = None
    for k, h, w in levels(*prev.shape):
        R0, R1 = polyexp(level_image(prev, k, h, w)), polyexp(level_image(cur, k, h, w))
        flow = np.zeros((h, w, 2)) if flow is None else flow_up(flow, h, w)
        M = matrices(R0, R1, flow)
        for i in range(ITERATIONS):
            flow = blur_solve(M)
            if i + 1 < ITERATIONS:
                M = matrices(R0, R1, flow)
    return flow


def region(gt_shape, sr_shape):
    """(h, w): the common top-left rectangle of two frame shapes; ValueError below 32 x 32."""
    h, w = min(gt_shape[-2], sr_shape[-2]), min(gt_shape[-1], sr_shape[-1])
    levels(h, w)
    return h, w


def epe(a: np.ndarray, b: np.ndarray) -> float:
    d = a - b
    return float(np.mean(np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])))


def tof(gt: np.ndarray, sr: np.ndarray) -> np.ndarray:
    """uint8 [T,Hg,Wg] and [T,Hs,Ws] -> fp64 [T]; frame 0's previous frame is frame 0 itself (computed, not set to 0)."""
    if gt.ndim != 3 or sr.ndim != 3 or len(gt) != len(sr) or gt.dtype != np.uint8 or sr.dtype != np.uint8:
        raise ValueError("two uint8 stacks [T,H,W] of one length expected")
    h, w = region(gt.shape, sr.shape)
    gt, sr = gt[:, :h, :w], sr[:, :h, :w]
    return np.array([epe(farneback(gt[max(t - 1, 0)], gt[t]), farneback(sr[max(t - 1, 0)], sr[t])) for t in range(len(gt))])
