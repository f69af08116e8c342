"""Developer benchmark (GPU box only): `cdfo_amd.loss.lpips_loss` alone, forward and backward timed separately by events, with a seeded
random trunk of the published widths (metrics.lpips_random_params):

    python tools/bench_lpips_loss.py [N H W] [--passes 5]

Each pass is one forward and one backward, so the two forms alternate; the figures are the medians over the passes behind one warm-up
pass.  Also printed: the bytes held between forward and backward (the allocator's count across the forward, and the docstring's
formula), and the split of the backward by kind of launch."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def main():
    argv = list(sys.argv[1:])
    passes = 5
    if "--passes" in argv:
        at = argv.index("--passes")
        passes = int(argv[at + 1])
        del argv[at:at + 2]
    N, H, W = (int(a) for a in argv[:3]) if len(argv) >= 3 else (20, 256, 256)
    from cdfo_amd import metrics as M
    from cdfo_amd.loss import lpips_loss
    params = M.lpips_random_params()
    g = torch.Generator(device="cuda").manual_seed(1)
    hr = torch.rand(N, 1, H, W, device="cuda", generator=g)
    sr = (hr + 0.1 * torch.randn(N, 1, H, W, device="cuda", generator=g)).requires_grad_(True)
    kept = 4 * N * sum((H >> k) * (W >> k) * c * (n + 1) for k, (c, n) in enumerate(zip(params.widths, M.LPIPS_STAGES)))
    fwd, bwd = [], []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for it in range(passes + 1):
        sr.grad = None
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        ev[0].record()
        loss = lpips_loss(sr, hr, params)
        ev[1].record()
        held = torch.cuda.memory_allocated() - before
        loss.sum().backward()
        ev[2].record()
        torch.cuda.synchronize()
        if it:
            fwd.append(ev[0].elapsed_time(ev[1]))
            bwd.append(ev[1].elapsed_time(ev[2]))
    print(f"lpips_loss {N}x1x{H}x{W}, widths {params.widths}: forward {statistics.median(fwd):.2f} ms (passes {min(fwd):.2f} - {max(fwd):.2f}), "
          f"backward {statistics.median(bwd):.2f} ms ({min(bwd):.2f} - {max(bwd):.2f}), medians of {passes}")
    print(f"held between forward and backward: {held / 2**20:.1f} MiB by the allocator's count, {kept / 2**20:.1f} MiB by the formula; "
          f"peak allocated {torch.cuda.max_memory_allocated() / 2**20:.1f} MiB")


if __name__ == "__main__":
    main()
