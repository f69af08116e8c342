"""Developer benchmark (GPU box only) of the evaluation loop, cdfo_amd.evaluate:

    python tools/bench_evaluate.py [--size T H W] [--chunk K] [--repeats R]     sequence benchmark
    python tools/bench_evaluate.py --ssim [--frames N]                          the two SSIM kernels at 1080 x 1920

Sequence benchmark, one process, one warm-up pass then R passes each, medians: run_chunked alone; evaluate_sequence with metrics
only; with metrics and PNG writing at 8 and 16 workers; and the per-chunk times of the finish kernel and the two 8-bit metric
kernels from events.  --ssim: the separable 8-bit SSIM kernel (cdfo_metric_partials_u8) against ssim_kernel (cdfo_metric_partials)
on fp32 copies of the same frames, median of five."""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def _arg(name, n, default):
    if name not in sys.argv:
        return default
    k = sys.argv.index(name)
    v = [int(x) for x in sys.argv[k + 1:k + 1 + n]]
    return v if n > 1 else v[0]


def _median_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), ms


def ssim_ab():
    from cdfo_amd import metrics as M
    n = _arg("--frames", 1, 1)
    g = torch.Generator().manual_seed(0)
    a = torch.randint(0, 256, (n, 1080, 1920), generator=g, dtype=torch.uint8).cuda()
    b = (a.float() + torch.randn(a.shape, device="cuda") * 8).clamp(0, 255).round().to(torch.uint8)
    af, bf = a.float(), b.float()
    new, _ = _median_ms(lambda: M.ssim_u8(a, b, 4))
    old, _ = _median_ms(lambda: M.calculate_ssim(af, bf, 4, from_unit_range=False))
    d = (M.ssim_u8(a, b, 4) - M.calculate_ssim(af, bf, 4, from_unit_range=False)).abs().max().item()
    print(f"SSIM, {n} frame(s) of 1080x1920, crop 4, median of 5: separable 8-bit kernel {new:.3f} ms, fp32 121-tap kernel {old:.3f} ms "
          f"(x{old / new:.1f}); max |difference| of the two results {d:.2e}", flush=True)


def sequence():
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    from cdfo_amd.evaluate import evaluate_sequence, write_synthetic_sequence
    from cdfo_amd.priors import load_sequence
    from cdfo_amd.streaming import StreamingSR
    T, H, W = _arg("--size", 3, [64, 270, 480])
    chunk, reps = _arg("--chunk", 1, 8), _arg("--repeats", 1, 5)
    model = CVSR_V8().cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        lr, side, gt = write_synthetic_sequence(tmp, T, H, W)
        seq = load_sequence(lr, side)
        s = StreamingSR(model, seq["lr"], seq["pms"], seq["rms"], seq["ufs"], seq["mvl0"], seq["mvl1"])
        s.run_chunked(chunk)
        fps = []
        for _ in range(reps):
            s.run_chunked(chunk)
            fps.append(s.fps)
        print(f"run_chunked(chunk={chunk}) alone, {T} frames {H}x{W}: frames/s per pass {' '.join('%.2f' % f for f in fps)}; median "
              f"{np.median(fps):.2f}", flush=True)
        base = float(np.median(fps))
        del s
        for label, kw in (("metrics only", dict()), ("metrics + PNGs, 8 workers", dict(save=True, workers=8)),
                          ("metrics + PNGs, 16 workers", dict(save=True, workers=16))):
            save = os.path.join(tmp, "out") if kw.pop("save", False) else None
            run = lambda: evaluate_sequence(model, lr, side, gt_dir=gt, save_dir=save, chunk=chunk, **kw)
            run()
            rs = [run() for _ in range(reps)]
            fwd, tot = [r.frames / r.seconds_forward for r in rs], [r.frames / r.seconds_total for r in rs]
            print(f"evaluate_sequence, {label}: forward-only frames/s median {np.median(fwd):.2f}; end to end (files read included) "
                  f"per pass {' '.join('%.2f' % f for f in tot)}; median {np.median(tot):.2f} ({np.median(tot) / base:.3f} of run_chunked "
                  f"alone)", flush=True)
        # the three kernels on one chunk's worth of frames, from events
        out = torch.rand((chunk, 1, 4 * ((H + 7) // 8 * 8), 4 * ((W + 7) // 8 * 8)), device="cuda") * 1.2 - 0.1
        gt8 = torch.randint(0, 256, (chunk, 4 * H, 4 * W), dtype=torch.uint8).cuda()
        u8, _ = K.finish_frames(out, H, W, gt=gt8)
        fin, _ = _median_ms(lambda: K.finish_frames(out, H, W, gt=gt8, dst=u8))
        sq, _ = _median_ms(lambda: M.sse_u8(u8, gt8, 4))
        ss, _ = _median_ms(lambda: M.ssim_u8(u8, gt8, 4))
        print(f"per chunk of {chunk} frames {4 * H}x{4 * W} (wrapper included), median of 5: finish_frames with SSE {fin:.3f} ms, "
              f"8-bit squared-difference kernel {sq:.3f} ms, 8-bit SSIM kernel {ss:.3f} ms", flush=True)


if __name__ == "__main__":
    ssim_ab() if "--ssim" in sys.argv else sequence()
