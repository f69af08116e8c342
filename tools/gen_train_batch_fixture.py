"""Write tests/golden/train_batch_ref.npz from the REAL reference's training transforms (run once, on the CPU; no test runs it).

    python tools/gen_train_batch_fixture.py --reference DIR

Imports DIR/opt/data_LD_bi.py (``skimage`` is only used by its file reader and is stubbed when absent), builds one synthetic sample of
seven frames, H = 12, W = 16 (unfiltered planes H + 2 rows; motion-field reference components in 0..3, so zeros occur under zero and
non-zero vectors) and runs ``RandomCrop(8) -> Augment() -> ToTensor()`` plus the training script's ``permute`` and ``/32``
(train_LD_37.py:365-374) for all eight flag combinations at two crop origins.  The random draws are scripted for the duration of each
call: ``np.random.randint`` hands out (top, left), ``random.random`` the three flag draws.  The file holds data only: the inputs, the
plans (rows as ``ClipSet.batch`` takes them) and the seven outputs per case."""
import argparse
import importlib
import os
import random
import sys
import types

import numpy as np
import torch

H, W, CROP = 12, 16, 8
ORIGINS = ((0, 3), (4, 8))          # (top, left): an odd offset, and the far corner


def _import_reference(root):
    for name in ("skimage", "skimage.io", "skimage.transform", "pandas", "PIL", "PIL.Image"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
            if "." in name:
                setattr(sys.modules[name.split(".")[0]], name.split(".")[1], sys.modules[name])
    sys.path.insert(0, root)
    return importlib.import_module("opt.data_LD_bi")


def _sample(rs):
    mv = rs.randint(-128, 128, (1, H, W, 3)).astype(np.int8)
    mv[..., 2] = rs.randint(0, 4, (1, H, W))
    mv[0, ::3, ::2, :2] = 0                                        # zero vectors, under zero and non-zero reference components
    return dict(lr=rs.randint(0, 256, (7, H, W)).astype(np.uint8), pms=rs.randint(0, 256, (7, H, W)).astype(np.uint8),
                rms=rs.randint(-128, 128, (7, H, W)).astype(np.int8), ufs=rs.randint(0, 256, (7, H + 2, W)).astype(np.uint8),
                mvl0=mv, mvl1=rs.randint(-128, 128, (1, H, W, 3)).astype(np.int8),
                hr=rs.randint(0, 256, (1, 4 * H, 4 * W)).astype(np.uint8))


def _run(ref, d, top, left, flags):
    sample = {'lr_imgs': d["lr"], 'hr_imgs': d["hr"], 'mvl0s': d["mvl0"], 'mvl1s': d["mvl1"], 'mpm_s': d["pms"], 'pred_fs': None,
              'unflt_fs': d["ufs"], 'res_s': d["rms"], 'qp': None, 'lrbi': None}
    ints, draws = iter((top, left)), iter(0.25 if f else 0.75 for f in flags)
    keep = np.random.randint, random.random
    np.random.randint, random.random = (lambda *a, **k: next(ints)), (lambda: next(draws))
    try:
        data = ref.ToTensor()(ref.Augment()(ref.RandomCrop(CROP)(sample)))
    finally:
        np.random.randint, random.random = keep
    data = {k: v[None] for k, v in data.items()}                   # the DataLoader's batch dimension
    return dict(x=data['lr_imgs'].permute(0, 2, 1, 3, 4), mvs0=data['mvl0s'].permute(0, 2, 1, 3, 4).contiguous() / 32.0,
                mvs1=data['mvl1s'].permute(0, 2, 1, 3, 4).contiguous() / 32.0, rms=data['res_s'],
                pms=data['mpm_s'].permute(0, 2, 1, 3, 4).contiguous(), hr=data['hr_imgs'][:, :, 0], ufs=data['unflt_fs'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                  "train_batch_ref.npz"))
    args = ap.parse_args()
    ref = _import_reference(args.reference)
    d = _sample(np.random.RandomState(20))
    plans, outs = [], {}
    for top, left in ORIGINS:
        for bits in range(8):
            hf, vf, rot = bits & 1, (bits >> 1) & 1, (bits >> 2) & 1
            plans.append((0, 0, top, left, hf, vf, rot, 0))
            with np.errstate(divide="ignore", invalid="ignore"):
                for k, v in _run(ref, {k: v.copy() for k, v in d.items()}, top, left, (hf, vf, rot)).items():
                    outs.setdefault(k, []).append(v.contiguous().numpy().astype(np.float32)[0])
    out = {"out_" + k: np.stack(v) for k, v in outs.items()}
    assert np.isinf(out["out_mvs0"]).any() and not np.isnan(out["out_mvs0"]).any()
    np.savez_compressed(args.out, plans=np.array(plans, np.int32), crop=np.int32(CROP),
                        **{"in_" + k: v for k, v in d.items() if k != "mvl1"}, **out)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
