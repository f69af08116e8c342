"""Evaluate one sequence end to end (cdfo_amd.evaluate.evaluate_sequence; the reference's eval_seq, test_LD_37.py:115-206):

    python tools/eval_sequence.py --lr LR_DIR --side SIDE_DIR [--gt GT_DIR] [--out SAVE_DIR] [--chunk 8] [--share] [--workers 8]
                                  [--weights FILE.pth] [--name SEQUENCE]
    python tools/eval_sequence.py --synthetic T H W [--out SAVE_DIR] ...

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
    a = ap.parse_args()
    if a.synthetic is None and not (a.lr and a.side):
        ap.error("--lr and --side, or --synthetic T H W")
    import torch
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd.evaluate import evaluate_sequence, format_log, write_synthetic_sequence
    model = CVSR_V8()
    if a.weights:
        model.load_state_dict(torch.load(a.weights, map_location="cpu"))
    model = model.cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        lr, side, gt = a.lr, a.side, a.gt
        if a.synthetic is not None:
            lr, side, gt = write_synthetic_sequence(tmp, *a.synthetic)
        r = evaluate_sequence(model, lr, side, gt_dir=gt, save_dir=a.out, chunk=a.chunk, share_compensation=a.share, workers=a.workers)
    name = a.name or os.path.basename(os.path.normpath(lr if a.synthetic is None else "synthetic"))
    if gt is not None:
        print(format_log(r, name))
    print(f"{name}: {r.frames} frames, chunk {a.chunk}{', shared compensation' if a.share else ''}: "
          f"{r.frames / r.seconds_forward:.2f} frames/s forward only, {r.frames / r.seconds_total:.2f} frames/s end to end "
          f"(files read, metrics{', PNGs written with ' + str(a.workers) + ' workers' if a.out else ''})")


if __name__ == "__main__":
    main()
