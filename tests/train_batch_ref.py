"""The numpy statement of a training batch (cdfo_amd/train_data.py, csrc/train_batch.hip): the reference's
``RandomCrop -> Augment -> ToTensor`` (opt/data_LD_bi.py) followed by the training script's ``permute`` and ``/32``
(train_LD_37.py:365-374), written from their semantics, one correctly rounded fp32 operation per step.

A plan row is ``(seq, first, top, left, hflip, vflip, rot, 0)``.  For an n x n output plane cut at (top, left):

    out[y][x] = P[top + i'][left + j'] / 255,   (i, j) = (x, y) if rot else (y, x),   i' = n-1-i if vflip,   j' = n-1-j if hflip

(the flips act on the crop, the transposition comes last).  The motion field of the centre frame goes through the same index
map; its first two components are swapped, negated with the flips, swapped again by the transposition, divided by ``-ref``
(NaN -> 0, an infinity stays) and spread over the seven slots with the weights 3, 2, 1, 0, -1, -2, -3, over 128."""
import numpy as np

W7 = (3.0, 2.0, 1.0, 0.0, -1.0, -2.0, -3.0)


def index_map(n, top, left, hf, vf, rot):
    """(rows, cols) int arrays [n,n]: the source position of every output position."""
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    i, j = (x, y) if rot else (y, x)
    return top + (n - 1 - i if vf else i), left + (n - 1 - j if hf else j)


def plane(P, n, top, left, hf, vf, rot):
    r, c = index_map(n, top, left, hf, vf, rot)
    return P[r, c].astype(np.float32) / np.float32(255.0)


def flows(mv, n, top, left, hf, vf, rot):
    """mv: one frame's field [H,W,3] (a, b, ref) -> [7,2,n,n] fp32."""
    r, c = index_map(n, top, left, hf, vf, rot)
    g = mv[r, c].astype(np.float32)
    m0, m1 = g[..., 1], g[..., 0]
    if hf:
        m0 = -m0
    if vf:
        m1 = -m1
    if rot:
        m0, m1 = m1, m0
    den = g[..., 2] * np.float32(-1.0)
    out = np.zeros((7, 2, n, n), np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for q, m in enumerate((m0, m1)):
            p = m / den
            p = np.where(np.isnan(p), np.float32(0.0), p).astype(np.float32)
            for k, w in enumerate(W7):
                if k != 3:
                    out[k, q] = (p * np.float32(w)) / np.float32(128.0)
    return out


def batch(lr, pms, rms, ufs, mvl0, hr, plan, crop):
    """The seven tensors of ``ClipSet.batch`` as numpy arrays, from the set's arrays [S,T,...] and a plan [B,8]."""
    plan = np.asarray(plan)
    B, c = plan.shape[0], crop
    out = dict(x=np.zeros((B, 7, 1, c, c), np.float32), mvs0=np.zeros((B, 7, 2, c, c), np.float32),
               mvs1=np.zeros((B, 7, 2, c, c), np.float32), pms=np.zeros((B, 7, 1, c, c), np.float32),
               rms=np.zeros((B, 1, 7, c, c), np.float32), ufs=np.zeros((B, 1, 7, c, c), np.float32),
               hr=np.zeros((B, 1, 4 * c, 4 * c), np.float32))
    for b, (s, f, top, left, hf, vf, rot, _) in enumerate(plan.tolist()):
        for k in range(7):
            out["x"][b, k, 0] = plane(lr[s, f + k], c, top, left, hf, vf, rot)
            out["pms"][b, k, 0] = plane(pms[s, f + k], c, top, left, hf, vf, rot)
            out["rms"][b, 0, k] = plane(rms[s, f + k], c, top, left, hf, vf, rot)
            out["ufs"][b, 0, k] = plane(ufs[s, f + k], c, top, left, hf, vf, rot)
        out["hr"][b, 0] = plane(hr[s, f + 3], 4 * c, 4 * top, 4 * left, hf, vf, rot)
        out["mvs0"][b] = flows(mvl0[s, f + 3], c, top, left, hf, vf, rot)
    return out
