"""Write tests/golden/niqe_ref.npz from the REAL reference's NIQE (run once, on the CPU; no test runs it).

    python tools/gen_niqe_fixture.py --reference DIR

Imports DIR/metric/niqe.py (torch, scipy and PIL) and runs ``calculate_niqe(u / 255 as [1,1,H,W] float32)`` with
DIR/metric/weight/niqe_modelparameters.mat on six seeded 8-bit frames, blurred noise plus white noise scaled to 0 .. 255:

    a  96 x 192   1 x 2 blocks: the smallest covariance with two rows, no crop
    b  200 x 300  region 192 x 288, 2 x 3 blocks: padding must clamp at the region, not the frame; the block order
    c  192 x 288  with u[80:192, :112] = 77: block (1, 0) and the 16 samples around it are flat, so its MSCN samples are one constant
                  at both scales (NaN features, alphas gam[0], index 0 on NaN); with only the block itself flat the windows at its
                  edge see the neighbours and no feature is NaN
    d  297 x 401  region 288 x 384, contrast stretched so that large areas clip at 0 and 255
    e  96 x 96    one block: a zero covariance
    f  200 x 300  a second frame of b's size (the GPU tests launch b, c and f together)

The reference's per-block features of both scales are hooked out of its ``blockproc`` (block (ih, iw) at row iw * nh + ih).  The file
holds data only: the two model arrays, the frames, the features [nb,36] and the score per frame."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

NAMES = "abcdef"


def _blur(x, taps):
    g = np.exp(-0.5 * (np.arange(-taps, taps + 1) / (taps / 2.0)) ** 2)
    g /= g.sum()
    for axis in (0, 1):
        x = np.apply_along_axis(lambda v: np.convolve(np.pad(v, taps, mode="reflect"), g, mode="valid"), axis, x)
    return x


def _frame(rs, H, W, gain=1.0):
    x = 6.0 * _blur(rs.randn(H, W), 4) + 0.35 * rs.randn(H, W)
    x = (x - x.mean()) / x.std()
    return np.clip(np.rint(127.5 + gain * 42.0 * x), 0, 255).astype(np.uint8)


def frames():
    rs = np.random.RandomState(96)
    f = dict(a=_frame(rs, 96, 192), b=_frame(rs, 200, 300), c=_frame(rs, 192, 288), d=_frame(rs, 297, 401, 4.0), e=_frame(rs, 96, 96),
             f=_frame(rs, 200, 300))
    f["c"][80:192, :112] = 77
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                  "niqe_ref.npz"))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    ref = importlib.import_module("metric.niqe")
    import scipy.io
    model = os.path.join(args.reference, "metric", "weight", "niqe_modelparameters.mat")
    params = scipy.io.loadmat(model)
    out = dict(mu_prisparam=np.ravel(params["mu_prisparam"]).astype(np.float64), cov_prisparam=params["cov_prisparam"].astype(np.float64))
    seen, inner = [], ref.blockproc

    def hooked(*a, **k):
        r = inner(*a, **k)
        seen.append(r[0].numpy().copy())                            # [nb,18] of the one frame
        return r

    ref.blockproc = hooked
    for name, u in frames().items():
        del seen[:]
        with torch.no_grad():
            s = ref.calculate_niqe(torch.from_numpy(u.astype(np.float32) / np.float32(255.0))[None, None], pretrained_model_path=model)
        assert len(seen) == 2 and np.isfinite(float(s)), (name, len(seen), s)
        F = np.concatenate(seen, axis=1).astype(np.float64)
        flat = np.isnan(F).any(axis=1)
        assert flat.sum() == (1 if name == "c" else 0), (name, flat)
        out["frame_" + name], out["features_" + name], out["score_" + name] = u, F, np.float64(float(s))
        print(name, u.shape, F.shape, "clipped %.2f" % np.mean((u == 0) | (u == 255)), "score %.6f" % float(s))
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
