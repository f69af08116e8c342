"""Developer micro-benchmark (GPU box only): DualAttAlignment's statistics at the headline's group shape, 24 x 272 x 480.

  one pass    kernels.align_stats (kf never written): reads warped, pred, xc once = 3T, T = one [24,272,480,64] fp32 tensor
  four passes the launches it replaces: kf = conv1x1([warped, pred]) (2T read, T written), gram_partial(xc, kf) (2T read),
              chan_sum_partial(warped), chan_sum_partial(pred) (T read each)
and the folded convolution with its channel sums from the epilogue against conv + chan_sum_partial(o).
Each line: time, algorithmic bytes (what the pass has to move), GB/s.  usage: python tools/bench_align_stats.py [B H W]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cdfo_amd import kernels as K


def timeit(fn, n=10):
    fn(); fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    B, H, W = (int(v) for v in sys.argv[1:4]) if len(sys.argv) >= 4 else (24, 272, 480)
    T = 4.0 * B * H * W * 64
    warped, pred, xc = (torch.randn(B, H, W, 64, device="cuda") for _ in range(3))
    pc = K.pack_conv(torch.randn(64, 128, 1, 1, device="cuda") / 128 ** 0.5, None)
    fold = K.PackedConv(torch.randn(B, 192 * 64, device="cuda") / 14, None, 64, 192, 1, 64, False, 192 * 64)
    kf = K.empty_act(B, H, W, 64, "cuda")
    o = K.empty_act(B, H, W, 64, "cuda")
    rows = [
        ("align_stats (one pass)", 3 * T, lambda: K.align_stats(warped, pred, xc, pc, K.ACT_RELU, 16)),
        ("  conv1x1 -> kf", 3 * T, lambda: K.conv([warped, pred], pc, act=K.ACT_RELU, out=kf, prec=K.PREC_BF16X3)),
        ("  gram_partial(xc, kf)", 2 * T, lambda: K.gram_partial(xc, kf, 16)),
        ("  chan_sum_partial(warped)", T, lambda: K.chan_sum_partial(warped)),
        ("  chan_sum_partial(pred)", T, lambda: K.chan_sum_partial(pred)),
        ("folded conv + channel sums", 4 * T, lambda: K.conv([warped, pred, xc], fold, act=K.ACT_RELU, out=o, prec=K.PREC_BF16X3, chan_sum_out=True)),
        ("  folded conv", 4 * T, lambda: K.conv([warped, pred, xc], fold, act=K.ACT_RELU, out=o, prec=K.PREC_BF16X3)),
        ("  chan_sum_partial(o)", T, lambda: K.chan_sum_partial(o)),
    ]
    ms = {}
    for name, by, fn in rows:
        ms[name] = timeit(fn)
        print(f"{name:30s} {ms[name]:7.3f} ms  {by / 1e9:6.2f} GB  {by / ms[name] / 1e6:7.1f} GB/s", flush=True)
    four = sum(ms[r[0]] for r in rows[1:5])
    print(f"statistics: one pass {ms[rows[0][0]]:.3f} ms (3T floor at 6.29 TB/s: {3 * T / 6.29e9:.3f} ms), four passes {four:.3f} ms")
    print(f"folded conv: with sums {ms[rows[5][0]]:.3f} ms, conv + chan_sum_partial {ms[rows[6][0]] + ms[rows[7][0]]:.3f} ms")


if __name__ == "__main__":
    main()
