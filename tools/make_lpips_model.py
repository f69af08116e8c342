"""Write the model file `--lpips` takes (cdfo_amd.metrics.lpips_params) from a user's own torch checkpoints:

    python tools/make_lpips_model.py --trunk VGG16.pth --lins LINS.pth --out model.npz

--trunk: a state dict with VGG16's ``features.{0,2,5,7,10,12,14,17,19,21,24,26,28}.weight`` / ``.bias`` (further entries, the
classifier's for instance, are ignored).  --lins: a state dict with ``lin{0..4}.model.1.weight`` ([1,C,1,1] each), the learned
per-channel weights of the distance.  The output holds ``w0`` .. ``w12``, ``b0`` .. ``b12`` (fp32) and ``lin0`` .. ``lin4`` (fp64).  Only
``torch.load`` and numpy are used: neither the ``lpips`` package nor torchvision is needed, and the project ships no model of its own."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main():
    from cdfo_amd import metrics as M
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trunk", required=True, help="the trunk's checkpoint (a torch state dict)")
    ap.add_argument("--lins", required=True, help="the head's checkpoint (a torch state dict)")
    ap.add_argument("--out", required=True, help="the .npz to write")
    a = ap.parse_args()
    params = M.lpips_params((a.trunk, a.lins))
    np.savez(a.out, **params.arrays())
    print(f"{a.out}: stage widths {params.widths}, {sum(w.size + b.size for w, b in zip(params.weights, params.biases))} trunk parameters, "
          f"{sum(l.size for l in params.lins)} lin weights")


if __name__ == "__main__":
    main()
