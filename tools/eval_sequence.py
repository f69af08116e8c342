"""Evaluate one sequence end to end (cdfo_amd.evaluate.evaluate_sequence; the reference's eval_seq, test_LD_37.py:115-206):

    python tools/eval_sequence.py --lr LR_DIR --side SIDE_DIR [--gt GT_DIR] [--out SAVE_DIR] [--chunk 8] [--share] [--workers 8]
                                  [--weights FILE.pth] [--name SEQUENCE] [--msssim] [--niqe PARAMS] [--brisque MODEL] [--tof]
                                  [--lpips MODEL] [--rescale-metrics]
    python tools/eval_sequence.py --synthetic T H W [--out SAVE_DIR] ...
    python tools/eval_sequence.py --lr-yuv FILE --size W H --side SIDE_DIR [--gt-yuv FILE [--gt-size W H]] [--out-yuv FILE] ...
    python tools/eval_sequence.py --synthetic T H W --yuv [--out-yuv FILE] ...

The last two forms read and write raw 8-bit YUV 4:2:0 (I420) files (cdfo_amd.evaluate.evaluate_yuv): the luma goes through the model,
the chroma is upsampled x4 on the device, PSNR is reported for Y, U and V.  The ground truth is 4W x 4H unless --gt-size says otherwise.
--pix-fmt NAME (ffmpeg's names: gray, yuv420p, yuv444p and their 10le / 12le / 16le forms) gives the one format of the three files.
--msssim (any form, with ground truth): five-scale MS-SSIM of the luma as well, `` MS-SSIM: %.5f`` behind the log line; the region
compared must be at least 176 samples each way.
--niqe PARAMS (any 8-bit form, WITH OR WITHOUT ground truth): the no-reference metric NIQE of every output frame's luma against the
pristine model in PARAMS, an .npz with mu_prisparam [36] and cov_prisparam [36,36] or the MATLAB file the reference ships
(cdfo_amd.metrics.niqe_params; the project ships no model); `` NIQE: %.5f`` behind the log line, or a line of its own without ground truth.
--brisque MODEL (any 8-bit form, with or without ground truth): the no-reference metric BRISQUE of every output frame's luma with the
support-vector model in MODEL, an .npz with sv [n,36], sv_coef [n], feature_ranges [36,2], gamma and rho (cdfo_amd.metrics.brisque_params;
the project ships no model, tools/gen_brisque_fixture.py --model-out writes one from a copy of the reference); `` BRISQUE: %.5f`` last on
the log line, or on the line of its own.
--tof (any 8-bit form, with ground truth): the temporal-consistency figure tOF, the mean distance between the Farneback flow of consecutive
ground-truth frames and that of consecutive result frames (cdfo_amd.metrics.tof_u8; the definition is the project's own, cv2 parity
unpinned); `` tOF: %.5f`` last on the log line.  The common region must be at least 32 x 32.
--lpips MODEL (any 8-bit form, with ground truth): LPIPS, the learned perceptual distance of every result frame's luma to the ground
truth through a VGG-shaped trunk (cdfo_amd.metrics.lpips_u8), with the model in MODEL, an .npz with w0 .. w12, b0 .. b12 and lin0 ..
lin4 (cdfo_amd.metrics.lpips_params; the project ships no model, tools/make_lpips_model.py writes one from a user's checkpoints;
parity with the lpips package is unpinned); `` LPIPS: %.5f`` last on the log line.  The common region must be at least 16 x 16.
--rescale-metrics (with --pix-fmt above 8 bits): --niqe, --brisque, --tof and --lpips are no error there but run their 16-bit forms on
the luma, a sample v of the format's peak read as 255 v / peak (LPIPS: v / peak); the project's own definition, the
reference has none above 8 bits.  On 8-bit material it changes nothing.

Prints the reference's log line and frames/s, forward only and end to end.  --synthetic writes a random sequence of T frames of
H x W with 4H x 4W ground truth into a temporary directory and evaluates that (with --weights absent the model is randomly
initialised: the figures say how fast, not how good)."""
import argparse
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lr")
    ap.add_argument("--side")
    ap.add_argument("--gt")
    ap.add_argument("--out")
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--share", action="store_true", help="run_chunked's share_compensation=True (opt-in, see cdfo_amd/streaming.py)")
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--weights")
    ap.add_argument("--name")
    ap.add_argument("--synthetic", type=int, nargs=3, metavar=("T", "H", "W"))
    ap.add_argument("--lr-yuv")
    ap.add_argument("--size", type=int, nargs=2, metavar=("W", "H"))
    ap.add_argument("--gt-yuv")
    ap.add_argument("--gt-size", type=int, nargs=2, metavar=("W", "H"))
    ap.add_argument("--out-yuv")
    ap.add_argument("--yuv", action="store_true", help="with --synthetic: write the sequence as I420 files and run evaluate_yuv")
    ap.add_argument("--msssim", action="store_true", help="report the luma's five-scale MS-SSIM as well (needs ground truth)")
    ap.add_argument("--niqe", metavar="PARAMS", help="score every output frame with NIQE against this pristine model (.npz or .mat)")
    ap.add_argument("--brisque", metavar="MODEL", help="score every output frame with BRISQUE with this support-vector model (.npz)")
    ap.add_argument("--tof", action="store_true", help="report the luma's tOF (Farneback flow of result against ground truth) as well")
    ap.add_argument("--lpips", metavar="MODEL", help="report the luma's LPIPS against the ground truth with this model (.npz) as well")
    ap.add_argument("--rescale-metrics", action="store_true",
                    help="above 8 bits: run --niqe / --brisque / --tof / --lpips on the luma read as 255 v / peak instead of refusing")
    ap.add_argument("--pix-fmt", default="yuv420p", help="the format of the raw files (cdfo_amd.yuv.parse_pix_fmt); default yuv420p")
    ap.add_argument("--coding", choices=("LD", "RA"), default="LD",
                    help="RA: flows from both motion lists, for a model trained on the random-access field (--synthetic then marks blocks)")
    a = ap.parse_args()
    yuv = a.lr_yuv is not None or a.yuv
    if a.lr_yuv is not None and not (a.size and a.side):
        ap.error("--lr-yuv needs --size W H and --side")
    if a.yuv and a.synthetic is None:
        ap.error("--yuv goes with --synthetic T H W")
    if a.pix_fmt != "yuv420p" and not yuv:
        ap.error("--pix-fmt goes with --lr-yuv or --synthetic T H W --yuv")
    if a.synthetic is None and not yuv and not (a.lr and a.side):
        ap.error("--lr and --side, or --lr-yuv, --size and --side, or --synthetic T H W")
    import torch
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd.evaluate import (evaluate_sequence, evaluate_yuv, format_log, format_log_yuv, write_synthetic_sequence,
                                   write_synthetic_sequence_yuv)
    model = CVSR_V8()
    if a.weights:
        model.load_state_dict(torch.load(a.weights, map_location="cpu"))
    model = model.cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        if yuv:
            lr, side, gt, size = a.lr_yuv, a.side, a.gt_yuv, a.size
            if a.synthetic is not None:
                T, H, W = a.synthetic
                (lr, side, gt), size = write_synthetic_sequence_yuv(tmp, T, H, W, pix_fmt=a.pix_fmt, markers=a.coding == "RA"), (W, H)
            r = evaluate_yuv(model, lr, size[0], size[1], side, gt_yuv=gt, save_yuv=a.out_yuv, chunk=a.chunk,
                             share_compensation=a.share, workers=a.workers, gt_size=tuple(a.gt_size) if a.gt_size else None,
                             pix_fmt=a.pix_fmt, msssim=a.msssim, niqe=a.niqe, brisque=a.brisque, tof=a.tof, lpips=a.lpips,
                             coding=a.coding, rescale_metrics=a.rescale_metrics)
        else:
            lr, side, gt = a.lr, a.side, a.gt
            if a.synthetic is not None:
                lr, side, gt = write_synthetic_sequence(tmp, *a.synthetic, markers=a.coding == "RA")
            r = evaluate_sequence(model, lr, side, gt_dir=gt, save_dir=a.out, chunk=a.chunk, share_compensation=a.share,
                                  workers=a.workers, msssim=a.msssim, niqe=a.niqe, brisque=a.brisque, tof=a.tof, lpips=a.lpips,
                                  coding=a.coding, rescale_metrics=a.rescale_metrics)
    name = a.name or os.path.basename(os.path.normpath(lr if a.synthetic is None else "synthetic"))
    if gt is not None:
        print(format_log_yuv(r, name) if yuv else format_log(r, name))
    elif a.niqe or a.brisque:
        print(name + ' Average' + ''.join(' %s: %.5f' % (k, v) for k, v, on in (("NIQE", r.mean_niqe, a.niqe), ("BRISQUE", r.mean_brisque, a.brisque))
                                          if on))
    written = ""
    if yuv and a.out_yuv:
        written = ", I420 file written" if a.pix_fmt == "yuv420p" else f", {a.pix_fmt} file written"
    elif a.out and not yuv:
        written = f", PNGs written with {a.workers} workers"
    print(f"{name}: {r.frames} frames, chunk {a.chunk}{', shared compensation' if a.share else ''}: "
          f"{r.frames / r.seconds_forward:.2f} frames/s forward only, {r.frames / r.seconds_total:.2f} frames/s end to end "
          f"(files read, metrics{written})")


if __name__ == "__main__":
    main()
