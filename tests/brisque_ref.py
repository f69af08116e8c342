"""ORACLE (test infrastructure only): the fp64 numpy statement of the project's BRISQUE, on one 8-bit luma frame.

The luma is the frame itself, x = u as fp64, H, W >= 16.  Per scale: the MSCN map under the 7x7 window of `window()` with ZERO
padding at the edge of the frame and the reference's fp32 epsilon 2^-23 under the root; the symmetric fit of the map over all its
samples (`r_ggd`, the inverse table); the four products with a partner taken circularly over the WHOLE frame, `np.roll` by
(0,1), (1,0), (1,1), (-1,1), each fitted asymmetrically (`r_gam`, NIQE's table).  Scale 2 reads the half-size image: the fixed 8
taps of `HALF_TAPS` on x itself (no / 255), down the columns and then along the rows, the edge sample repeated, ceil(n / 2) outputs,
fp64 and not rounded.  Score: the features scaled to -1 .. 1 by the model's ranges, an RBF support-vector sum, minus rho.  A fit that
is undefined (no sample of one sign, all samples zero) gives NaN, a NaN distance picks table index 0; the reference asserts instead."""
import functools
import math
import os

import numpy as np

SHIFTS = ((0, 1), (1, 0), (1, 1), (-1, 1))
HALF_TAPS = np.array([-3, -9, 29, 111, 111, 29, -9, -3], np.float64) / 256.0
MIN_SIZE = 16


def window() -> np.ndarray:
    """fspecial(7, 7/6): exp(-(x^2 + y^2) / (2 sigma^2)), entries below eps * max zeroed, normalised, ROUNDED TO fp32, widened."""
    sigma = 7.0 / 6
    y, x = np.ogrid[-3.0:4.0, -3.0:4.0]
    h = np.exp(-(x * x + y * y) / (2.0 * sigma * sigma))
    h[h < np.finfo(np.float64).eps * h.max()] = 0
    h /= h.sum()
    return h.astype(np.float32).astype(np.float64)


def table():
    """(gam, r_gam, r_ggd) fp64 [9801]: gam = torch's float32 arange(0.2, 10.001, 0.001) widened (the one line of torch here, as in
    niqe_ref.table), r_gam = exp(2 lgamma(2/g) - (lgamma(1/g) + lgamma(3/g))), r_ggd = exp(lgamma(1/g) + lgamma(3/g) - 2 lgamma(2/g))."""
    import torch
    gam = torch.arange(0.2, 10 + 0.001, 0.001).numpy().astype(np.float64)
    r_gam = np.array([math.exp(2 * math.lgamma(2.0 / g) - (math.lgamma(1.0 / g) + math.lgamma(3.0 / g))) for g in gam])
    r_ggd = np.array([math.exp(math.lgamma(1.0 / g) + math.lgamma(3.0 / g) - 2 * math.lgamma(2.0 / g)) for g in gam])
    return gam, r_gam, r_ggd


def luma(u: np.ndarray) -> np.ndarray:
    if u.ndim != 2 or min(u.shape) < MIN_SIZE:
        raise ValueError(f"BRISQUE needs at least {MIN_SIZE} x {MIN_SIZE} samples, got {u.shape}")
    return u.astype(np.float64)


def mscn(img: np.ndarray) -> np.ndarray:
    h = window()
    H, W = img.shape
    p = np.pad(img, 3, mode="constant")
    q = p * p
    mu, sq = np.zeros_like(img), np.zeros_like(img)
    for i in range(7):
        for j in range(7):
            mu = mu + h[i, j] * p[i:i + H, j:j + W]
            sq = sq + h[i, j] * q[i:i + H, j:j + W]
    sigma = np.sqrt(np.abs(sq - mu * mu) + 2.0 ** -23)
    return (img - mu) / (sigma + 1.0)


def _half_rows(t: np.ndarray) -> np.ndarray:
    n = t.shape[0]
    m = (n + 1) // 2
    p = np.concatenate([t[2::-1], t, t[:n - 5:-1]], axis=0)          # [a,b,c,..] -> [c,b,a,a,b,c,..]: the edge sample repeated
    out = np.zeros((m,) + t.shape[1:], np.float64)
    for k in range(8):
        out = out + HALF_TAPS[k] * p[k:k + 2 * m:2]                   # output i reads inputs 2i-3 .. 2i+4
    return out


def half(img: np.ndarray) -> np.ndarray:
    return _half_rows(_half_rows(img).T).T


def products(m: np.ndarray):
    """The five maps: m and its four products with the circular partner."""
    return [m] + [m * np.roll(m, s, axis=(0, 1)) for s in SHIFTS]


def sums(m: np.ndarray) -> np.ndarray:
    """fp64 [5,6] of an MSCN map: per map (count < 0, count > 0, sum v^2 over < 0, over > 0, sum |v|, sum v^2)."""
    out = np.zeros((5, 6), np.float64)
    for k, v in enumerate(products(m)):
        neg, pos = v < 0, v > 0
        out[k] = (neg.sum(), pos.sum(), (v[neg] ** 2).sum(), (v[pos] ** 2).sum(), np.abs(v).sum(), (v ** 2).sum())
    return out


def search(x: float, row: np.ndarray):
    """(index, gap): the first minimum of |row - x| (0 for NaN) and the relative gap between the two best distances."""
    if math.isnan(x):
        return 0, float("inf")
    d = np.abs(row - x)
    i = int(np.argmin(d))
    two = np.partition(d, 1)[:2]
    return i, float((two[1] - two[0]) / max(two[1], 1e-300))


def features_from_sums(s: np.ndarray, n: int, tab=None):
    """(fp64 [18] features, int [5] table indices, fp64 [5] gaps) of one scale from its sums [5,6] over n samples."""
    gam, r_gam, r_ggd = tab or table()
    F, I, G = np.zeros(18), np.zeros(5, np.int64), np.zeros(5)
    with np.errstate(divide="ignore", invalid="ignore"):
        s2, E = s[0, 5] / n, s[0, 4] / n
        I[0], G[0] = search(float(s2 / (E * E)), r_ggd)
        F[:2] = gam[I[0]], s2
        for k in range(1, 5):
            ls, rs = np.sqrt(s[k, 2] / s[k, 0]), np.sqrt(s[k, 3] / s[k, 1])
            g = ls / rs
            ma = s[k, 4] / n
            rhat = ma * ma / (s[k, 5] / n)
            g2 = g * g + 1.0
            rn = rhat * (g * g * g + 1.0) * (g + 1.0) / (g2 * g2)
            I[k], G[k] = search(float(rn), r_gam)
            a = float(gam[I[k]])
            eta = (rs - ls) * math.exp(math.lgamma(2 / a) - (math.lgamma(1 / a) + math.lgamma(3 / a)) / 2)
            F[4 * k - 2:4 * k + 2] = a, eta, ls * ls, rs * rs
    return F, I, G


def pieces(u: np.ndarray, tab=None) -> dict:
    """Every intermediate of one frame: the two MSCN maps, the half image, the sums [2,5,6], indices and gaps [2,5], features [36]."""
    tab = tab or table()
    img = luma(u)
    m1, hf = mscn(img), half(img)
    m2 = mscn(hf)
    s1, s2 = sums(m1), sums(m2)
    (f1, i1, g1), (f2, i2, g2) = features_from_sums(s1, m1.size, tab), features_from_sums(s2, m2.size, tab)
    return dict(mscn1=m1, half=hf, mscn2=m2, sums1=s1, sums2=s2, index=np.stack([i1, i2]), gap=np.stack([g1, g2]),
                features=np.concatenate([f1, f2]))


def features(u: np.ndarray, tab=None) -> np.ndarray:
    return pieces(u, tab)["features"]


def score(F, sv, sv_coef, ranges, gamma, rho) -> float:
    F, ranges = np.asarray(F, np.float64), np.asarray(ranges, np.float64)
    z = -1.0 + 2.0 * (F - ranges[:, 0]) / (ranges[:, 1] - ranges[:, 0])
    d = ((z[None, :] - np.asarray(sv, np.float64)) ** 2).sum(axis=1)
    return float((np.asarray(sv_coef, np.float64).ravel() * np.exp(-float(gamma) * d)).sum() - float(rho))


def brisque(u: np.ndarray, model, tab=None) -> float:
    return score(features(u, tab), *model)


# ---- the committed fixture (tools/gen_brisque_fixture.py) and the statement's results on it, computed once per process and shared ----
FRAMES = "abcde"                                                       # the frames the reference scored; "z" is all zeros
SIZES = dict(a=(16, 16), b=(37, 83), c=(70, 130), d=(70, 130), z=(70, 130), e=(96, 160))
ALPHAS = tuple(s + a for s in (0, 18) for a in (0, 2, 6, 10, 14))      # the columns that hold entries of gam


@functools.lru_cache(None)
def golden() -> dict:
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "brisque_ref.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(None)
def shared_table():
    return table()


@functools.lru_cache(None)
def golden_pieces(name: str) -> dict:
    """`pieces` of fixture frame ``name``; read-only for every test."""
    return pieces(golden()["frame_" + name], shared_table())


def model(as_reference: bool = False):
    """(sv, sv_coef, feature_ranges, gamma, rho) of the fixture, fp64.  ``as_reference``: the ranges and the two scalars rounded to
    fp32 and widened, the way the reference holds them beside its float32 features (the support vectors are stored in fp32 already)."""
    z = golden()
    m = [z["sv"].astype(np.float64), z["sv_coef"].astype(np.float64).ravel(), z["feature_ranges"].astype(np.float64),
         np.float64(z["gamma"]), np.float64(z["rho"])]
    if as_reference:
        m[2:] = [np.asarray(x).astype(np.float32).astype(np.float64) for x in m[2:]]
    return tuple(m)


def perturbation_bound(name: str, rel: float = 1e-9, draws: int = 100) -> float:
    """10 x the largest change of the statement's score of frame ``name`` when every feature moves by ``rel`` relative with a random
    sign, over ``draws`` seeded draws: what features within ``rel`` of the statement's may cost the score."""
    F, m = golden_pieces(name)["features"], model()
    rs, s0, worst = np.random.RandomState(FRAMES.index(name)), score(F, *m), 0.0
    for _ in range(draws):
        worst = max(worst, abs(score(F * (1.0 + rel * rs.choice([-1.0, 1.0], size=F.shape)), *m) - s0))
    return 10.0 * worst
