"""Train CVSR_V8 on a clip set resident on the device (cdfo_amd.train.fit; the loop of train_LD_37.py:359-402 and train_RA_37.py):

    python tools/train.py --seq LR_DIR SIDE_DIR HR_DIR [--seq ...] --out DIR [--coding LD] [--epochs 30000] [--batch-size 20] [--crop 64]
                          [--lr 1e-4] [--weight-decay 1e-5] [--val-itv 200] [--val LR_DIR SIDE_DIR GT_DIR] [--val-coding LD] [--weights FILE.pth]
                          [--lpips MODEL|random --lpips-weight W] [--ffl-weight W [--ffl-alpha A]]
                          [--ssim-weight W [--ssim-scales 1|5]]
                          [--optimizer torch|device] [--max-grad-norm X] [--deterministic] [--save-state] [--resume STATE.pth]
    python tools/train.py --synthetic S T H W --out DIR ...

--coding RA trains the random-access configuration: the clip set keeps both motion lists (the mvl1 files beside mvl0) and the flow field
is built from both (opt/data_RA_bi.py); --batch-size and --val-itv then default to 24 and 400 as in train_RA_37.py.

--lpips MODEL adds the perceptual term to the step's loss, charbonnier + W * sum of the batch's per-frame LPIPS (cdfo_amd.loss.lpips_loss):
MODEL is the caller's .npz (tools/make_lpips_model.py; the project ships none), `random` a seeded random trunk of the published widths,
which says that the loop runs and nothing about quality.  --lpips-weight W is then required, finite and positive.

--ffl-weight W adds the frequency term, W * sum of the batch's per-frame focal frequency loss (cdfo_amd.loss.focal_frequency_loss: the
spectrum of sr - hr weighted by its own magnitude to the power --ffl-alpha, default 1); --crop must then be a power of two from 4 to 128.

--ssim-weight W adds the structural term, W * sum of the batch's per-frame 1 - SSIM (cdfo_amd.loss.ssim_loss; --crop >= 3) or, with
--ssim-scales 5, 1 - MS-SSIM over five scales (cdfo_amd.loss.msssim_loss; --crop >= 44: the HR crop must hold 176 samples each way).

--optimizer device runs Adam on the device (cdfo_amd.optim.DeviceAdam: three launches a step, the epoch's line gains the mean gradient
norm, a step with a non-finite gradient is skipped and counted instead of ending the run); --max-grad-norm X then clips the gradient to
that norm.  --save-state writes ckpt/epoch-N.state.pth beside every epoch-N.pth: the optimizer's state, the generators' states, the
averages and the run's arguments.  --resume ckpt/epoch-N.state.pth continues that run at epoch N with the weights of its sibling
epoch-N.pth (--weights is then not used); the run-defining arguments must be those of the run that wrote it.  With --deterministic
(or an LPIPS or FFL term) the continued run leaves the bits of the uninterrupted one.

--seq names one training sequence in the layout of cdfo_amd/priors.py (every frame with its own prior files, 00000 included) and a
directory of 8-bit grey HR frames %05d.png.  --synthetic trains on S random sequences of T frames of H x W instead
(cdfo_amd.train_data.synthetic_arrays): the figures say that the loop runs, not how good the model gets."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seq", nargs=3, action="append", metavar=("LR_DIR", "SIDE_DIR", "HR_DIR"))
    ap.add_argument("--synthetic", type=int, nargs=4, metavar=("S", "T", "H", "W"))
    ap.add_argument("--out", required=True)
    ap.add_argument("--epochs", type=int, default=30000)
    ap.add_argument("--coding", choices=("LD", "RA"), default="LD")
    ap.add_argument("--batch-size", type=int, help="default: 20 (LD), 24 (RA)")
    ap.add_argument("--crop", type=int, default=64)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--weight-decay", type=float, default=1e-5)
    ap.add_argument("--val-itv", type=int, help="default: 200 (LD), 400 (RA)")
    ap.add_argument("--val", nargs=3, metavar=("LR_DIR", "SIDE_DIR", "GT_DIR"))
    ap.add_argument("--val-coding", choices=("LD", "RA"), default="LD",
                    help="the flows of the --val evaluation: LD (the reference's, list 1 alone) or RA (the field --coding RA trains on)")
    ap.add_argument("--weights")
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--lpips", metavar="MODEL|random", help="an LPIPS model (.npz) or `random`: adds --lpips-weight * LPIPS to the loss")
    ap.add_argument("--lpips-weight", type=float, default=0.0)
    ap.add_argument("--ffl-weight", type=float, default=0.0, help="adds --ffl-weight * the focal frequency loss to the step's loss")
    ap.add_argument("--ffl-alpha", type=float, default=1.0, help="the exponent of the spectrum weight (needs --ffl-weight)")
    ap.add_argument("--ssim-weight", type=float, default=0.0, help="adds --ssim-weight * (1 - SSIM) of every frame to the step's loss")
    ap.add_argument("--ssim-scales", type=int, choices=(1, 5), default=1, help="5: 1 - MS-SSIM instead (needs --ssim-weight)")
    ap.add_argument("--optimizer", choices=("torch", "device"), default="torch", help="device: Adam in HIP (cdfo_amd.optim.DeviceAdam)")
    ap.add_argument("--max-grad-norm", type=float, help="clip the gradient to this norm (needs --optimizer device)")
    ap.add_argument("--deterministic", action="store_true", help="a reproducible run: the flow warp's adjoint adds in a fixed order")
    ap.add_argument("--save-state", action="store_true", help="write ckpt/epoch-N.state.pth beside every checkpoint")
    ap.add_argument("--resume", metavar="STATE.pth", help="continue the run of this state file (ckpt/epoch-N.state.pth)")
    a = ap.parse_args()
    if (a.seq is None) == (a.synthetic is None):
        ap.error("--seq LR_DIR SIDE_DIR HR_DIR (once per sequence), or --synthetic S T H W")
    if a.batch_size is None:
        a.batch_size = 24 if a.coding == "RA" else 20
    if a.val_itv is None:
        a.val_itv = 400 if a.coding == "RA" else 200
    import torch
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd.train import fit
    from cdfo_amd.train_data import ClipSet, synthetic_arrays
    from cdfo_amd import metrics
    lpips = None if a.lpips is None else metrics.lpips_random_params() if a.lpips == "random" else metrics.lpips_params(a.lpips)
    torch.manual_seed(a.seed)
    model = CVSR_V8(SCGs=8)
    if a.weights and not a.resume:
        model.load_state_dict(torch.load(a.weights, map_location="cpu"))
    model = model.cuda()
    if a.synthetic:
        six, mvl1 = synthetic_arrays(*a.synthetic, seed=a.seed, coding=a.coding), None
        if a.coding == "RA":
            *six, mvl1 = six
        clips = ClipSet.from_arrays(*six, mvl1=mvl1, coding=a.coding)
    else:
        clips = ClipSet.from_directories(a.seq, coding=a.coding)
    print(f"{clips.coding}: {len(clips)} sequences of {clips.T} frames of {clips.H}x{clips.W} on the device")
    fit(model, clips, a.epochs, a.out, batch_size=a.batch_size, crop=a.crop, lr=a.lr, weight_decay=a.weight_decay, val_itv=a.val_itv,
        val=a.val, seed=a.seed, val_coding=a.val_coding, lpips=lpips, lpips_weight=a.lpips_weight, ffl_weight=a.ffl_weight,
        ffl_alpha=a.ffl_alpha, optimizer=a.optimizer, max_grad_norm=a.max_grad_norm, deterministic=a.deterministic, save_state=a.save_state,
        resume=a.resume, ssim_weight=a.ssim_weight, ssim_scales=a.ssim_scales)


if __name__ == "__main__":
    main()
