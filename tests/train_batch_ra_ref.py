"""The numpy statement of a random-access training batch (cdfo_amd/train_data.py with ``coding="RA"``, csrc/train_batch.hip:
cdfo_train_batch_ra): the reference's ``RandomCrop -> Augment -> ToTensor`` of opt/data_RA_bi.py followed by the training script's
``permute`` and ``/32`` (train_RA_37.py:383-386), written from their semantics, one correctly rounded fp32 operation per step.

The planes and the index map are tests/train_batch_ref.py's.  Both lists' fields of the centre frame go through that map and through
the LD statement's component rules (``m0 = b``, ``m1 = a``; hflip negates ``m0``, vflip ``m1``, rot swaps them).  Then, per pixel,

    p2 = m(list 0) / (ref0 * -1)          NaN -> +0, an infinity stays
    p4 = m(list 1) / ref1                 NaN -> +0, an infinity stays
    ref0 == -99:  p2 = -p4
    ref1 == -99:  p4 = -p2                (p2 after the line above: with both marked p4 is unchanged and p2 = -p4)

and slots 0, 1, 2 hold ``fl(p2 * w) / 128`` with w = 3, 2, 1, slot 3 is +0, slots 4, 5, 6 hold ``fl(p4 * w) / 128`` with w = 1, 2, 3.
The negations make ``-0``; the reference's output carries them, so comparisons are made on bit patterns (`bits`)."""
import numpy as np

import train_batch_ref as R

MARK = -99


def bits(a):
    """The fp32 array's bit patterns: equality that sees a zero's sign (and would see a NaN's payload)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def flows(mv0, mv1, n, top, left, hf, vf, rot):
    """mv0, mv1: one frame's fields [H,W,3] (a, b, ref) of the two lists -> [7,2,n,n] fp32."""
    r, c = R.index_map(n, top, left, hf, vf, rot)
    p = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for mv, sign in ((mv0, np.float32(-1.0)), (mv1, None)):
            g = mv[r, c].astype(np.float32)
            m0, m1 = g[..., 1], g[..., 0]
            if hf:
                m0 = -m0
            if vf:
                m1 = -m1
            if rot:
                m0, m1 = m1, m0
            den = g[..., 2] if sign is None else g[..., 2] * sign
            q = np.stack([m0 / den, m1 / den]).astype(np.float32)
            p.append(np.where(np.isnan(q), np.float32(0.0), q))
    p2, p4 = p
    no0, no1 = mv0[r, c][..., 2] == MARK, mv1[r, c][..., 2] == MARK
    p2 = np.where(no0, -p4, p2)
    p4 = np.where(no1, -p2, p4)
    out = np.zeros((7, 2, n, n), np.float32)
    for k, src, w in ((0, p2, 3.0), (1, p2, 2.0), (2, p2, 1.0), (4, p4, 1.0), (5, p4, 2.0), (6, p4, 3.0)):
        out[k] = (src * np.float32(w)) / np.float32(128.0)
    return out


def marker_classes(mv0, mv1, n, top, left, hf, vf, rot):
    """The set of (list 0 marked, list 1 marked) pairs inside one cropped window."""
    r, c = R.index_map(n, top, left, hf, vf, rot)
    return set(zip((mv0[r, c][..., 2] == MARK).ravel().tolist(), (mv1[r, c][..., 2] == MARK).ravel().tolist()))


def batch(lr, pms, rms, ufs, mvl0, mvl1, hr, plan, crop):
    """The seven tensors of an RA ``ClipSet.batch`` as numpy arrays: the LD statement's planes, the field above as mvs0 and mvs1."""
    out = R.batch(lr, pms, rms, ufs, mvl0, hr, plan, crop)
    for b, (s, f, top, left, hf, vf, rot, _) in enumerate(np.asarray(plan).tolist()):
        out["mvs0"][b] = flows(mvl0[s, f + 3], mvl1[s, f + 3], crop, top, left, hf, vf, rot)
    out["mvs1"] = out["mvs0"].copy()
    return out
