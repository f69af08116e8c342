"""ORACLE (test infrastructure only): the fp64 numpy statement of the project's MS-SSIM, on one pair of frames.

Level 0: the common size less ``crop`` on every side.  Level j + 1: the 2x2 non-overlapping mean of level j from its top-left sample,
a trailing odd row or column dropped; no padding anywhere.  Per level, with the 11-tap Gaussian of oracle/metrics_ref.py over valid
positions only: M_cs = mean(cs), M_ssim = mean(l * cs).  Combined: prod_{j<4} max(M_cs[j], 0)^w[j] * max(M_ssim[4], 0)^w[4]."""
import numpy as np

from oracle.metrics_ref import _filter_valid, gaussian_kernel_11

WEIGHTS = np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333])        # Wang, Simoncelli, Bovik 2003
MIN_SIZE = 176


def pool2(x: np.ndarray) -> np.ndarray:
    H, W = x.shape[0] // 2 * 2, x.shape[1] // 2 * 2
    return (x[0:H:2, 0:W:2] + x[0:H:2, 1:W:2] + x[1:H:2, 0:W:2] + x[1:H:2, 1:W:2]) / 4.0      # sums of integers / 4^j: exact


def level(a: np.ndarray, b: np.ndarray, peak: int):
    """(M_cs, M_ssim) of two fp64 planes."""
    C1, C2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
    g = gaussian_kernel_11()
    mu1, mu2 = _filter_valid(a, g), _filter_valid(b, g)
    s11 = _filter_valid(a * a, g) - mu1 ** 2
    s22 = _filter_valid(b * b, g) - mu2 ** 2
    s12 = _filter_valid(a * b, g) - mu1 * mu2
    cs = (2 * s12 + C2) / (s11 + s22 + C2)
    lum = (2 * mu1 * mu2 + C1) / (mu1 ** 2 + mu2 ** 2 + C1)
    return float(cs.mean()), float((lum * cs).mean())


def components(a: np.ndarray, b: np.ndarray, crop: int, peak: int) -> np.ndarray:
    """fp64 [5,2]: (M_cs, M_ssim) per level of two integer frames, compared over their common size less ``crop``."""
    H, W = min(a.shape[0], b.shape[0]), min(a.shape[1], b.shape[1])
    a, b = (x[crop:H - crop, crop:W - crop].astype(np.float64) for x in (a, b))
    if min(a.shape) < MIN_SIZE:
        raise ValueError(f"MS-SSIM needs {MIN_SIZE} samples each way, got {a.shape}")
    out = np.zeros((5, 2), np.float64)
    for j in range(5):
        out[j] = level(a, b, peak)
        a, b = pool2(a), pool2(b)
    return out


def combine(c: np.ndarray) -> float:
    c = np.asarray(c, dtype=np.float64)
    m = np.maximum(np.append(c[:4, 0], c[4, 1]), 0.0)
    return float(np.prod(m ** WEIGHTS))


def propagated_bound(c: np.ndarray, tol: float) -> float:
    """First-order bound on the combined value's error when each mean is within ``tol``: tol * sum w[j] / m[j] (the value is <= 1)."""
    c = np.asarray(c, dtype=np.float64)
    return tol * float(np.sum(WEIGHTS / np.append(c[:4, 0], c[4, 1])))


def correlated_pair(N: int, shape, peak: int, sigma: float, seed: int = 1):
    """a uniform over 0 .. peak, b = clip(a + rint(sigma N(0,1))); frame 1 of b (where there is one) equals a's."""
    rs = np.random.RandomState(seed)
    kind = np.uint8 if peak <= 255 else np.uint16
    a = rs.randint(0, peak + 1, (N,) + tuple(shape)).astype(np.int64)
    b = np.clip(a + np.rint(sigma * rs.randn(N, *shape)).astype(np.int64), 0, peak)
    if N > 1:
        b[1] = a[1]
    return a.astype(kind), b.astype(kind)
