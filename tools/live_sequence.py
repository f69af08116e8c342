"""Super-resolve one sequence the way a decoder would deliver it (cdfo_amd.live.LiveSR): one frame and its prior files are read and
pushed at a time, frames come back as soon as their chunk can run, device memory does not grow with the sequence.

    python tools/live_sequence.py --lr LR_DIR --side SIDE_DIR [--out SAVE_DIR] [--chunk 8] [--share] [--weights FILE.pth]
    python tools/live_sequence.py --synthetic T H W [--out SAVE_DIR] ...

The layout is the reference's test layout (cdfo_amd/priors.py); the priors and the motion field of frame t are read from the files of
index max(1, t), as the reference's loop reads them.  --out writes every frame as an 8-bit PNG under its LR file name (truncating
quantisation through cdfo_finish_frames, the reference's writer).  Prints frames/s (forward only and end to end, file reading
included) and torch.cuda.max_memory_allocated.  --synthetic writes a random sequence into a temporary directory first (with --weights
absent the model is randomly initialised: the figures say how fast, not how good)."""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lr")
    ap.add_argument("--side")
    ap.add_argument("--out")
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--share", action="store_true", help="share_compensation=True (opt-in, see cdfo_amd/streaming.py)")
    ap.add_argument("--weights")
    ap.add_argument("--synthetic", type=int, nargs=3, metavar=("T", "H", "W"))
    ap.add_argument("--coding", choices=("LD", "RA"), default="LD",
                    help="RA: list 0's field is pushed as well and the flows come from both lists (--synthetic then marks blocks)")
    a = ap.parse_args()
    if a.synthetic is None and not (a.lr and a.side):
        ap.error("--lr and --side, or --synthetic T H W")
    import numpy as np
    import torch
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd import kernels as K
    from cdfo_amd.evaluate import write_synthetic_sequence
    from cdfo_amd.live import LiveSR
    from cdfo_amd.priors import read_gray_png, write_gray_png
    model = CVSR_V8()
    if a.weights:
        model.load_state_dict(torch.load(a.weights, map_location="cpu"))
    model = model.cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        lr_dir, side = a.lr, a.side
        if a.synthetic is not None:
            lr_dir, side, _ = write_synthetic_sequence(tmp, *a.synthetic, gt=False, markers=a.coding == "RA")
        names = sorted(n for n in os.listdir(lr_dir) if n.lower().endswith(".png"))
        if not names:
            raise FileNotFoundError(f"no PNG frames in {lr_dir}")
        if a.out:
            os.makedirs(a.out, exist_ok=True)

        def deliver(done):
            for i, frame in done:
                if a.out:
                    write_gray_png(os.path.join(a.out, names[i]), K.finish_frames(frame, s.H, s.W)[0][0].cpu().numpy())

        s = None
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for t, name in enumerate(names):
            lr = read_gray_png(os.path.join(lr_dir, name))
            i = "%05d" % max(1, t)
            pm = read_gray_png(os.path.join(side, "part_m", i + "_M_mask.png"))
            uf = read_gray_png(os.path.join(side, "unfiltered", i + "_unflt.png"))
            rm = np.load(os.path.join(side, "res", i + "_res.npy"))[:, :, 0]
            mv = np.load(os.path.join(side, "mvl1", i + "_mvl1.npy"))
            if s is None:
                s = LiveSR(model, lr.shape[0], lr.shape[1], chunk=a.chunk, share_compensation=a.share, coding=a.coding)
            mv0 = np.load(os.path.join(side, "mvl0", i + "_mvl0.npy")) if a.coding == "RA" else None
            deliver(s.push(lr, pm, rm, uf, mv, mv0))
        deliver(s.close())
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
    print(f"{len(names)} frames of {s.H}x{s.W} pushed one at a time, chunk {a.chunk}{', shared compensation' if a.share else ''}"
          f"{', coding RA' if a.coding == 'RA' else ''}: "
          f"{s.fps:.2f} frames/s forward only, {len(names) / total:.2f} frames/s end to end (files read"
          f"{', PNGs written' if a.out else ''}); rings of {s.ring_capacity} frames, {s.resident_bytes / 2 ** 20:.1f} MiB resident, "
          f"torch.cuda.max_memory_allocated {torch.cuda.max_memory_allocated() / 2 ** 20:.1f} MiB")


if __name__ == "__main__":
    main()
