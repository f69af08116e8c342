"""TEST INFRASTRUCTURE: a numpy restatement of csrc/ssim_loss.hip's tiling, with switchable defects.

It does what the kernels do, tile by tile: a tile of 16 x 32 valid positions stages 26 x 42 samples of both frames (zeros beyond the
frame), runs the window along x over the staged rows and then along y, and its sums are added tile by tile in index order; the
P/Q/R pass repeats that; the adjoint stages 26 x 42 map values around 16 x 32 samples (zeros beyond the maps), runs the window as the
full correlation, and adds a quarter of the coarser level's gradient.  The loss and each gradient element are rounded to fp32 once;
the upstream product is a second fp32 rounding.  Without a defect it meets every bound of tests/ssim_loss_cases.py; each name in
DEFECTS breaks one index, factor or constant the way a kernel could, and misses the bound of at least one case
(tests/test_ssim_loss_cpu.py says which)."""
import numpy as np

import ssim_loss_ref as ref
from oracle.metrics_ref import gaussian_kernel_11

TH, TW, TAPS, HALO = 16, 32, 11, 10
SH, SW = TH + HALO, TW + HALO
DEFECTS = ("halo-short",         # the staged tile is 25 x 41: its last row and column are missing
           "centre-off",         # the window starts one sample late
           "adjoint-valid",      # the adjoint keeps only samples whose eleven taps all lie inside the maps
           "adjoint-no-flip",    # the adjoint runs the window in the forward's direction (shows with an asymmetric window only)
           "skip-partial",       # a tile that is not full is not computed
           "pool-odd-row",       # a dropped odd row or column takes the last coarse row's or column's gradient
           "spread-one",         # the coarse gradient arrives whole instead of as a quarter
           "q-without-2",        # x Gt*Q instead of 2 x Gt*Q
           "c1-c2-swapped",
           "clamp-gradient",     # a clamped frame keeps the coefficients of its positive factors
           "level4-cs")          # level 4 enters the product with M_cs instead of M_ssim


def _stage(img, y0, x0, rows, cols):
    """zeros [SH + 1, SW + 1] with img[y0 : y0 + rows, x0 : x0 + cols] (where it exists) at the top-left."""
    out = np.zeros(img.shape[:-2] + (SH + 1, SW + 1))
    ya, yb, xa, xb = max(y0, 0), min(y0 + rows, img.shape[-2]), max(x0, 0), min(x0 + cols, img.shape[-1])
    if yb > ya and xb > xa:
        out[..., ya - y0:yb - y0, xa - x0:xb - x0] = img[..., ya:yb, xa:xb]
    return out


def _valid_passes(s, g, shift):
    """[..., SH + 1, SW + 1] -> [..., TH, TW]: along x over the staged rows, then along y, k = 0 .. 10 in order."""
    hp = sum(g[k] * s[..., :, k + shift:k + shift + TW] for k in range(TAPS))
    return sum(g[k] * hp[..., k + shift:k + shift + TH, :] for k in range(TAPS))


def _tiles(rows, cols, defects):
    for ty in range(-(-rows // TH)):
        for tx in range(-(-cols // TW)):
            if "skip-partial" in defects and ((ty + 1) * TH > rows or (tx + 1) * TW > cols):
                continue
            yield ty * TH, tx * TW


def _stats(x, y, g, defects):
    """Per tile: (oy0, ox0, rows, cols, m1, m2, e11, e22, e12) with the statistics cut to the rows x cols valid positions."""
    h, w = x.shape
    ho, wo = h - HALO, w - HALO
    short = 1 if "halo-short" in defects else 0
    shift = 1 if "centre-off" in defects else 0
    for oy0, ox0 in _tiles(ho, wo, defects):
        sx, sy = (_stage(a.astype(np.float64), oy0, ox0, SH - short, SW - short) for a in (x, y))
        rows, cols = min(TH, ho - oy0), min(TW, wo - ox0)
        yield (oy0, ox0, rows, cols) + tuple(_valid_passes(p, g, shift)[:rows, :cols] for p in (sx, sy, sx * sx, sy * sy, sx * sy))


def _cs_l(m1, m2, e11, e22, e12, C1, C2):
    B2, B1 = (e11 - m1 * m1) + (e22 - m2 * m2) + C2, m1 * m1 + m2 * m2 + C1
    return (2.0 * (e12 - m1 * m2) + C2) / B2, (2.0 * m1 * m2 + C1) / B1, B2, B1


def model(sr, hr, peak=1.0, levels=1, upstream=None, defects=(), g=None):
    """(loss fp32 [N], gradient fp32 [N,H,W] times ``upstream`` in fp32) of fp32 frames [N,H,W]."""
    defects = frozenset(defects)
    assert defects <= set(DEFECTS), defects
    g = np.asarray(gaussian_kernel_11() if g is None else g, dtype=np.float64)
    sr, hr = np.asarray(sr, np.float32), np.asarray(hr, np.float32)
    N = len(sr)
    up = np.ones(N, np.float32) if upstream is None else np.asarray(upstream, np.float32)
    C1, C2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
    if "c1-c2-swapped" in defects:
        C1, C2 = C2, C1
    loss, grad = np.zeros(N, np.float32), np.zeros(sr.shape, np.float32)
    for n in range(N):
        xs, ys = [sr[n]], [hr[n]]
        for j in range(1, levels):
            xs.append(ref.pool_numpy(xs[-1]))
            ys.append(ref.pool_numpy(ys[-1]))
        means = np.zeros((levels, 2))
        for j in range(levels):
            s = np.zeros(2)
            for _, _, _, _, *st in _stats(xs[j], ys[j], g, defects):
                cs, lum, _, _ = _cs_l(*st, C1, C2)
                s += (cs.sum(), (lum * cs).sum())
            means[j] = s / ((xs[j].shape[0] - HALO) * (xs[j].shape[1] - HALO))
        coef = np.zeros((levels, 2))
        if levels == 1:
            loss[n], coef[0, 1] = np.float32(1.0 - means[0, 1]), -1.0
        else:
            last = 0 if "level4-cs" in defects else 1
            used = np.append(means[:4, 0], means[4, last])
            clamped = bool((used <= 0).any())
            prod = 1.0 if clamped else float(np.prod(used ** ref.WEIGHTS))
            loss[n] = np.float32(1.0 if clamped else 1.0 - prod)
            d = np.zeros(5) if clamped else -ref.WEIGHTS * prod / used
            if clamped and "clamp-gradient" in defects:
                pos = used > 0
                d = np.where(pos, -ref.WEIGHTS * np.prod(used[pos] ** ref.WEIGHTS[pos]) / np.where(pos, used, 1.0), 0.0)
            coef[:4, 0], coef[4, last] = d[:4], d[4]
        coarse = None
        for j in range(levels - 1, -1, -1):
            x, y = xs[j].astype(np.float64), ys[j].astype(np.float64)
            h, w = x.shape
            ho, wo = h - HALO, w - HALO
            pqr = np.zeros((3, ho, wo))
            for oy0, ox0, rows, cols, m1, m2, e11, e22, e12 in _stats(xs[j], ys[j], g, defects):
                cs, lum, B2, B1 = _cs_l(m1, m2, e11, e22, e12, C1, C2)
                alpha, beta = (coef[j, 0] + coef[j, 1] * lum) / (ho * wo), coef[j, 1] * cs / (ho * wo)
                pqr[0, oy0:oy0 + rows, ox0:ox0 + cols] = alpha * ((2 * m1 * cs - 2 * m2) / B2) + beta * ((2 * m2 - 2 * m1 * lum) / B1)
                pqr[1, oy0:oy0 + rows, ox0:ox0 + cols] = -(alpha * cs / B2)
                pqr[2, oy0:oy0 + rows, ox0:ox0 + cols] = 2 * (alpha / B2)
            gl = np.zeros((h, w))
            for y0, x0 in _tiles(h, w, defects):
                sp = _stage(pqr, y0 - HALO, x0 - HALO, SH, SW)
                if "adjoint-no-flip" in defects:
                    t = _valid_passes(sp, g, 0)
                else:                                       # sample column x0 + c takes map columns x0 + c - k: staged column c + 10 - k
                    hq = sum(g[k] * sp[:, :, HALO - k:HALO - k + TW] for k in range(TAPS))
                    t = sum(g[k] * hq[:, HALO - k:HALO - k + TH, :] for k in range(TAPS))
                rows, cols = min(TH, h - y0), min(TW, w - x0)
                t = t[:, :rows, :cols]
                xt, yt = x[y0:y0 + rows, x0:x0 + cols], y[y0:y0 + rows, x0:x0 + cols]
                v = (t[0] + (1.0 if "q-without-2" in defects else 2.0) * xt * t[1]) + yt * t[2]
                if "adjoint-valid" in defects:
                    yy, xx = np.mgrid[y0:y0 + rows, x0:x0 + cols]
                    v = np.where((yy >= HALO) & (yy < ho) & (xx >= HALO) & (xx < wo), v, 0.0)
                if coarse is not None:
                    yy, xx = np.mgrid[y0:y0 + rows, x0:x0 + cols] >> 1
                    hc, wc = coarse.shape
                    if "pool-odd-row" in defects:
                        yy, xx = np.minimum(yy, hc - 1), np.minimum(xx, wc - 1)
                    ok = (yy < hc) & (xx < wc)
                    factor = 1.0 if "spread-one" in defects else 0.25
                    v = v + np.where(ok, factor * coarse[np.minimum(yy, hc - 1), np.minimum(xx, wc - 1)], 0.0)
                gl[y0:y0 + rows, x0:x0 + cols] = v
            coarse = gl
        grad[n] = up[n] * coarse.astype(np.float32)
    return loss, grad
