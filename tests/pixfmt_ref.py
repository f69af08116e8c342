"""References with a peak for the high-bit-depth tests (samples in 0 .. peak = 2**depth - 1), written out for the tests: nothing here
comes from the package.  PSNR and SSIM are oracle/metrics_ref.py's functions with `peak` in place of 255 (tests/test_pixfmt_cpu.py pins
them to the oracle at peak = 255); the chroma filter is tests/chroma_ref.py's integer sums clipped to [0, peak]; the quantiser is the
statement of cdfo_finish_frames_u16."""
import numpy as np

from chroma_ref import up4_sums


def calculate_psnr(img1, img2, crop_border, peak=255):
    a, b = img1.astype(np.float64), img2.astype(np.float64)
    if crop_border != 0:
        a = a[crop_border:-crop_border, crop_border:-crop_border, ...]
        b = b[crop_border:-crop_border, crop_border:-crop_border, ...]
    mse = np.mean((a - b) ** 2)
    return float("inf") if mse == 0 else 20.0 * np.log10(float(peak) / np.sqrt(mse))


def _filter_valid(img, g):
    H, W = img.shape
    tmp = np.zeros((H - 10, W), np.float64)
    for k in range(11):
        tmp += g[k] * img[k:k + H - 10, :]
    out = np.zeros((H - 10, W - 10), np.float64)
    for k in range(11):
        out += g[k] * tmp[:, k:k + W - 10]
    return out


def calculate_ssim(img1, img2, crop_border, peak=255):
    a, b = img1.astype(np.float64), img2.astype(np.float64)
    if crop_border != 0:
        a = a[crop_border:-crop_border, crop_border:-crop_border]
        b = b[crop_border:-crop_border, crop_border:-crop_border]
    C1, C2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 ** 2))
    g = g / g.sum()
    mu1, mu2 = _filter_valid(a, g), _filter_valid(b, g)
    s11 = _filter_valid(a * a, g) - mu1 ** 2
    s22 = _filter_valid(b * b, g) - mu2 ** 2
    s12 = _filter_valid(a * b, g) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s11 + s22 + C2))
    return float(m.mean())


def sample_dtype(peak):
    return np.uint8 if peak <= 255 else np.uint16


def up4(p, peak):
    """[..., h, w] samples -> [..., 4h, 4w]: clip((sums + 8192) >> 14, 0, peak), the shift arithmetic."""
    return np.ascontiguousarray(np.clip((up4_sums(p) + 8192) >> 14, 0, peak).astype(sample_dtype(peak)))


def quantise(x, mode, peak):
    """clip to [0,1] (NaN -> 0), one fp32 multiply by peak, truncation / round-half-even."""
    v = np.where(np.isnan(x), np.float32(0), x.astype(np.float32))
    v = np.clip(v, np.float32(0), np.float32(1)) * np.float32(peak)
    assert v.dtype == np.float32
    return (np.rint(v) if mode == "nearest" else v).astype(sample_dtype(peak))


def sse(out, gt, crop):
    """int64 [N]: the sum of squared differences over the common size less `crop`."""
    hm, wm = min(out.shape[1], gt.shape[1]), min(out.shape[2], gt.shape[2])
    d = out[:, crop:hm - crop, crop:wm - crop].astype(np.int64) - gt[:, crop:hm - crop, crop:wm - crop].astype(np.int64)
    return (d * d).sum(axis=(1, 2))


def contents(shape, seed, peak):
    """tests/chroma_ref.py's three kinds of plane at a peak: random samples, a 0/peak checkerboard, random 0/peak."""
    rs = np.random.RandomState(seed)
    kind = sample_dtype(peak)
    yy, xx = np.indices(shape[-2:])
    board = np.broadcast_to((((yy + xx) % 2) * peak).astype(kind), shape).copy()
    return dict(random=rs.randint(0, peak + 1, shape).astype(kind), checkerboard=board,
                binary=(rs.randint(0, 2, shape) * peak).astype(kind))
