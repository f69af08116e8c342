"""The cases and the bounds of the SSIM / MS-SSIM loss tests (tests/test_ssim_loss_cpu.py, test_gpu_ssim_loss_kernels.py,
test_gpu_ssim_loss.py).

A case is (levels, H, W, N, sigma, peak): hr uniform in [0, 1], sr = clip(hr + sigma randn, 0, 1), both times peak, in fp32.
One scale: one window (11 x 11), one more column or row, 21 x 21 (a sample lies in 1 to 11 windows each way), two shapes with partial
tiles, and TILE_16x32 = 59 x 91: larger than the kernels' tile of 16 x 32 valid positions plus its halo of 10 both ways (26 x 42),
with a partial last tile both ways (49 = 3 * 16 + 1 rows, 81 = 2 * 32 + 17 columns of positions); N = 1 and 3, sigma 0.05 and 0.5, and
one case at peak 255.  Five scales: 176 x 176 (level 4 is one window), 177 x 191 (odd sizes at levels 0, 2 and 3: 191 -> 95 -> 47 ->
23 -> 11) and 200 x 233, N = 2.  Every one of a five-scale case's ten means of the fp64 statement is asserted >= 0.25 here (the
lowest is 0.442), so that no live case sits near the clamp; the clamp case is sr = 1 - hr at 176 x 176, whose M_cs is negative at levels 0 - 3.
`upstream(N)` is a non-unit upstream gradient per frame with a 0 for frame 1 of three, which must then get zeros.

The bounds are derived, not measured.  Behind the fp32 loads everything is fp64, whose error against the statement is below 1e-10
relative for samples in [0, peak] (121 * 2^-53 of cancellation residue over C2 / peak^2 = 9e-4, times small constants).  So:
    loss       |l - l64| <= 2^-23 |l64| + 1e-9         one fp32 rounding (2^-24), a factor two over it
    gradient   max |g - g64| <= 2^-22 max |g64|        per frame, upstream included: the element's rounding and the upstream
                                                       product's rounding (2^-24 each), a factor two over them
    sr == hr   |loss| <= 1e-9 and max |g| <= 1e-9 / peak."""
import functools

import numpy as np

import ssim_loss_ref as ref

TILE = (16, 32)
TILE_16x32 = (59, 91)
SSIM_SHAPES = ((11, 11), (11, 12), (12, 11), (21, 21), (43, 75), (64, 64), TILE_16x32)
MS_SHAPES = ((176, 176), (177, 191), (200, 233))
SIGMAS = (0.05, 0.5)
SSIM_CASES = tuple((1, h, w, n, s, 1.0) for h, w in SSIM_SHAPES for n in (1, 3) for s in SIGMAS) + ((1, 43, 75, 3, 0.05, 255.0),)
MS_CASES = tuple((5, h, w, 2, s, 1.0) for h, w in MS_SHAPES for s in SIGMAS)
CASES = SSIM_CASES + MS_CASES
CLAMP = (5, 176, 176, 2, "clamp", 1.0)
MEAN_FLOOR = 0.25


def case_id(c) -> str:
    return "L%d-%dx%d-n%d-s%s-p%g" % c


@functools.lru_cache(maxsize=None)
def case(c):
    """(sr, hr) fp32 [N,H,W], read-only."""
    levels, h, w, n, sigma, peak = c
    rs = np.random.RandomState(100000 * levels + 1000 * h + w + 17 * n + (3 if sigma == 0.5 else 0))
    hr = rs.uniform(0, 1, (n, h, w))
    sr = 1.0 - hr if sigma == "clamp" else np.clip(hr + sigma * rs.randn(n, h, w), 0, 1)
    sr, hr = (sr * peak).astype(np.float32), (hr * peak).astype(np.float32)
    sr.setflags(write=False)
    hr.setflags(write=False)
    return sr, hr


def upstream(n: int) -> np.ndarray:
    """A non-unit upstream gradient per frame; frame 1 of three gets 0."""
    return np.array([0.5, 1.75] if n == 2 else [0.5, 0.0, 2.0][:n], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def reference(c):
    """(loss fp64 [N], g fp64 [N,H,W] with `upstream` applied, means [N,levels,2], coef [N,levels,2]) of the fp64 statement, read-only."""
    levels, h, w, n, sigma, peak = c
    sr, hr = case(c)
    out = ref.statement(sr, hr, peak, levels, upstream(n).astype(np.float64))
    if levels == 5 and sigma != "clamp":                                     # one scale has no clamp to sit near
        assert out[2].min() >= MEAN_FLOOR, (case_id(c), out[2].min())
    for a in out:
        a.setflags(write=False)
    return out


def loss_bound(l64) -> np.ndarray:
    return 2.0 ** -23 * np.abs(l64) + 1e-9


def loss_ratio(loss, l64) -> float:
    """max over the frames of |l - l64| / bound."""
    return float((np.abs(np.asarray(loss, dtype=np.float64) - l64) / loss_bound(l64)).max())


def grad_ratio(g, g64) -> float:
    """max over the frames of max |g - g64| / (2^-22 max |g64|); a frame whose g64 is all zero gives 0 if g is, else inf."""
    e = np.abs(np.asarray(g, dtype=np.float64) - g64).reshape(len(g64), -1).max(axis=1)
    top = 2.0 ** -22 * np.abs(g64).reshape(len(g64), -1).max(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(top > 0, e / top, np.where(e == 0, 0.0, np.inf)).max())
