"""ORACLE (test infrastructure only): the fp64 numpy statement of the project's NIQE, on one 8-bit luma frame.

Region: the top-left 96 floor(H/96) x 96 floor(W/96).  MSCN with the 7x7 window of `window()` (its 49 two-dimensional values, rounded
to fp32 and widened), replicate padding at the edge of the REGION.  Half size: the fixed 8 taps of `HALF_TAPS` on img / 255.0, rows
first, then columns, the edge sample repeated, all in fp64, then * 255.0.  Block features of 96 x 96 (scale 1) and 48 x 48 (scale 2)
blocks, in the order block (ih, iw) -> row iw * nh + ih; the table search with `math.lgamma`.  Score: nanmean, the covariance of
the rows without NaN, the pseudo-inverse."""
import functools
import math
import os

import numpy as np

BLOCK = 96
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
HALF_TAPS = np.array([-3, -9, 29, 111, 111, 29, -9, -3], np.float64) / 256.0


def window() -> np.ndarray:
    """fspecial(7, 7/6): exp(-(x^2 + y^2) / (2 sigma^2)), entries below eps * max zeroed, normalised, ROUNDED TO fp32, widened."""
    sigma = 7.0 / 6
    y, x = np.ogrid[-3.0:4.0, -3.0:4.0]
    h = np.exp(-(x * x + y * y) / (2.0 * sigma * sigma))
    h[h < np.finfo(np.float64).eps * h.max()] = 0
    h /= h.sum()
    return h.astype(np.float32).astype(np.float64)


def table():
    """(gam, r_gam) fp64 [9801]: gam = the float32 arange(0.2, 10.001, 0.001) widened, r_gam = exp(2 lgamma(2/gam) - lgamma(1/gam) -
    lgamma(3/gam)).  The one line of torch here: its float32 arange steps in fp32 inside a vector, so 2158 of its entries are one fp32
    ulp away from numpy's float32(0.2 + 0.001 k), and the alphas ARE entries of this table."""
    import torch
    gam = torch.arange(0.2, 10 + 0.001, 0.001).numpy().astype(np.float64)
    r = np.array([math.exp(2 * math.lgamma(2.0 / g) - (math.lgamma(1.0 / g) + math.lgamma(3.0 / g))) for g in gam])
    return gam, r


def region(u: np.ndarray) -> np.ndarray:
    R, C = BLOCK * (u.shape[0] // BLOCK), BLOCK * (u.shape[1] // BLOCK)
    if R == 0 or C == 0:
        raise ValueError(f"NIQE needs at least {BLOCK} x {BLOCK} samples, got {u.shape}")
    return u[:R, :C].astype(np.float64)


def mscn(img: np.ndarray) -> np.ndarray:
    h = window()
    H, W = img.shape
    p = np.pad(img, 3, mode="edge")
    q = p * p
    mu, sq = np.zeros_like(img), np.zeros_like(img)
    for i in range(7):
        for j in range(7):
            mu = mu + h[i, j] * p[i:i + H, j:j + W]
            sq = sq + h[i, j] * q[i:i + H, j:j + W]
    sigma = np.sqrt(np.abs(sq - mu * mu) + 2.0 ** -52)
    return (img - mu) / (sigma + 1.0)


def _half_rows(t: np.ndarray) -> np.ndarray:
    n = t.shape[0]
    p = np.concatenate([t[2::-1], t, t[:n - 4:-1]], axis=0)          # [a,b,c,..] -> [c,b,a,a,b,c,..]: the edge sample repeated
    out = np.zeros((n // 2,) + t.shape[1:], np.float64)
    for k in range(8):
        out = out + HALF_TAPS[k] * p[k:k + n:2][:n // 2]              # output i reads inputs 2i-3 .. 2i+4
    return out


def half(img: np.ndarray) -> np.ndarray:
    t = img / 255.0
    t = _half_rows(t)
    t = _half_rows(t.T).T
    return t * 255.0


def block_sums(m: np.ndarray, B: int) -> np.ndarray:
    """fp64 [nb,5,6] of an MSCN map: per block and map (count < 0, count > 0, sum v^2 over < 0, over > 0, sum |v|, sum v^2)."""
    nh, nw = m.shape[0] // B, m.shape[1] // B
    out = np.zeros((nh * nw, 5, 6), np.float64)
    for iw in range(nw):
        for ih in range(nh):
            x = m[ih * B:(ih + 1) * B, iw * B:(iw + 1) * B]
            for k, v in enumerate([x] + [x * np.roll(x, s, axis=(0, 1)) for s in SHIFTS]):
                neg, pos = v < 0, v > 0
                out[iw * nh + ih, k] = (neg.sum(), pos.sum(), (v[neg] ** 2).sum(), (v[pos] ** 2).sum(), np.abs(v).sum(), (v ** 2).sum())
    return out


def search(rn: float, r_gam: np.ndarray):
    """(index, gap): the first minimum of |r_gam - rn| (0 for NaN) and the relative gap between the two best distances."""
    if math.isnan(rn):
        return 0, float("inf")
    d = np.abs(r_gam - rn)
    i = int(np.argmin(d))
    two = np.partition(d, 1)[:2]
    return i, float((two[1] - two[0]) / max(two[1], 1e-300))


def aggd(s: np.ndarray, n: int, tab):
    """(alpha, beta_l, beta_r, index, gap) from the six sums of one map of n samples."""
    gam, r_gam = tab
    with np.errstate(divide="ignore", invalid="ignore"):
        ls, rs = np.sqrt(s[2] / s[0]), np.sqrt(s[3] / s[1])
        g = ls / rs
        rhat = (s[4] / n) ** 2 / (s[5] / n)
        rn = rhat * (g ** 3 + 1) * (g + 1) / (g ** 2 + 1) ** 2
    i, gap = search(float(rn), r_gam)
    a = float(gam[i])
    c = math.sqrt(math.exp(math.lgamma(1 / a) - math.lgamma(3 / a)))
    return a, float(ls) * c, float(rs) * c, i, gap


def features_from_sums(sums: np.ndarray, n: int, tab=None):
    """(fp64 [nb,18] features, int [nb,5] table indices, fp64 [nb,5] gaps) of one scale."""
    tab = tab or table()
    F, I, G = np.zeros((len(sums), 18)), np.zeros((len(sums), 5), np.int64), np.zeros((len(sums), 5))
    for b, s in enumerate(sums):
        a, bl, br, I[b, 0], G[b, 0] = aggd(s[0], n, tab)
        F[b, :2] = a, (bl + br) / 2
        for k in range(1, 5):
            a, bl, br, I[b, k], G[b, k] = aggd(s[k], n, tab)
            F[b, 4 * k - 2:4 * k + 2] = a, (br - bl) * math.exp(math.lgamma(2 / a) - math.lgamma(1 / a)), bl, br
    return F, I, G


def pieces(u: np.ndarray, tab=None) -> dict:
    """Every intermediate of one frame: the two MSCN maps, the half image, the sums, indices and features [nb,36]."""
    tab = tab or table()
    img = region(u)
    m1, hf = mscn(img), half(img)
    m2 = mscn(hf)
    s1, s2 = block_sums(m1, BLOCK), block_sums(m2, BLOCK // 2)
    (f1, i1, g1), (f2, i2, g2) = features_from_sums(s1, BLOCK * BLOCK, tab), features_from_sums(s2, BLOCK * BLOCK // 4, tab)
    return dict(mscn1=m1, half=hf, mscn2=m2, sums1=s1, sums2=s2, index=np.stack([i1, i2]), gap=np.stack([g1, g2]),
                features=np.concatenate([f1, f2], axis=1))


def features(u: np.ndarray, tab=None) -> np.ndarray:
    return pieces(u, tab)["features"]


def score(F: np.ndarray, mu_pris: np.ndarray, cov_pris: np.ndarray) -> float:
    F = np.asarray(F, np.float64)
    nan = np.isnan(F)
    mu = np.where(nan, 0.0, F).sum(axis=0) / (~nan).sum(axis=0)
    rows = F[~nan.any(axis=1)]
    if len(rows) > 1:
        c = rows - rows.mean(axis=0)
        cov = c.T @ c / (len(rows) - 1)
    else:
        cov = np.zeros((F.shape[1], F.shape[1]))
    d = np.asarray(mu_pris, np.float64).ravel() - mu
    return float(np.sqrt(d @ np.linalg.pinv((np.asarray(cov_pris, np.float64) + cov) / 2) @ d))


def niqe(u: np.ndarray, mu_pris, cov_pris, tab=None) -> float:
    return score(features(u, tab), mu_pris, cov_pris)


# ---- the committed fixture (tools/gen_niqe_fixture.py) and the statement's results on it, computed once per process and shared ----
FRAMES = "abcdef"
ALPHAS = tuple(s + a for s in (0, 18) for a in (0, 2, 6, 10, 14))      # the columns that hold entries of gam


@functools.lru_cache(None)
def golden() -> dict:
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "niqe_ref.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(None)
def shared_table():
    return table()


@functools.lru_cache(None)
def golden_pieces(name: str) -> dict:
    """`pieces` of fixture frame ``name``; read-only for every test."""
    return pieces(golden()["frame_" + name], shared_table())


def model(as_reference: bool = False):
    """(mu, cov) of the fixture.  ``as_reference``: rounded to fp32 and widened, the way the reference holds them (it moves the
    model to the dtype of its float32 input before the fp64 arithmetic), so its recorded scores are those of the rounded model."""
    mu, cov = golden()["mu_prisparam"], golden()["cov_prisparam"]
    if as_reference:
        mu, cov = (x.astype(np.float32).astype(np.float64) for x in (mu, cov))
    return mu, cov


def perturbation_bound(name: str, rel: float = 1e-9, draws: int = 100) -> float:
    """10 x the largest change of the statement's score of frame ``name`` when every feature moves by ``rel`` relative with a random
    sign, over ``draws`` seeded draws: what features within ``rel`` of the statement's may cost the score."""
    F, (mu, cov) = golden_pieces(name)["features"], model()
    rs, s0, worst = np.random.RandomState(FRAMES.index(name)), score(golden_pieces(name)["features"], mu, cov), 0.0
    for _ in range(draws):
        worst = max(worst, abs(score(F * (1.0 + rel * rs.choice([-1.0, 1.0], size=F.shape)), mu, cov) - s0))
    return 10.0 * worst
