"""Developer benchmark (GPU box only) of the evaluation loop, cdfo_amd.evaluate:

    python tools/bench_evaluate.py [--size T H W] [--chunk K] [--repeats R]     sequence benchmark
    python tools/bench_evaluate.py --ssim [--frames N]                          the two SSIM kernels at 1080 x 1920
    python tools/bench_evaluate.py --yuv [--size T H W] [--chunk K] [--repeats R]    the PNG path against the raw 4:2:0 path
    python tools/bench_evaluate.py --yuv --pix-fmt NAME [--size T H W] ...           evaluate_yuv at NAME against 8-bit yuv420p
    python tools/bench_evaluate.py --msssim [--yuv] [--size T H W] [--chunk K] [--repeats R]    MS-SSIM: the kernels, and the option on / off
    python tools/bench_evaluate.py --niqe PARAMS [--yuv] [--size T H W] [--chunk K] [--repeats R]    NIQE: the kernels, and the option on / off
    python tools/bench_evaluate.py --brisque MODEL [--niqe PARAMS] [--yuv] [--size T H W] [--chunk K] [--repeats R]    BRISQUE likewise
    python tools/bench_evaluate.py --tof [--niqe PARAMS] [--yuv] [--size T H W] [--chunk K] [--repeats R]    tOF: the kernels, and the option on / off
    python tools/bench_evaluate.py --lpips MODEL|random [--yuv] [--size T H W] [--chunk K] [--repeats R] [--only kernels|evaluator]    LPIPS likewise
    python tools/bench_evaluate.py --rescale-metrics --yuv --pix-fmt NAME [--niqe PARAMS] [--brisque MODEL] [--tof] [--lpips MODEL|random]
                                   [--size T H W] [--chunk K] [--repeats R] [--only kernels|evaluator]    the four metrics above 8 bits

Sequence benchmark, one process, one warm-up pass then R passes each, medians: run_chunked alone; evaluate_sequence with metrics
only; with metrics and PNG writing at 8 and 16 workers; and the per-chunk times of the finish kernel and the two 8-bit metric
kernels from events.  --ssim: the separable 8-bit SSIM kernel (cdfo_metric_partials_u8) against ssim_kernel (cdfo_metric_partials)
on fp32 copies of the same frames, median of five.  --yuv: the same synthetic content once in the PNG layout and once as I420
files; run_chunked alone, then evaluate_sequence and evaluate_yuv end to end, metrics only and with the result written (the baseline
is the PNG path of this very run); the time the priors' PNGs and NPYs take to read, which both paths pay before their first chunk;
and chroma_up4 per chunk from events.  --yuv --pix-fmt NAME (a format of cdfo_amd/yuv.py): evaluate_yuv with metrics and the result
file, on 8-bit yuv420p and on NAME in the same process (the 8-bit run is the baseline), then the three 16-bit kernels against their
8-bit twins on one chunk of 1080 x 1920 frames, from events.  --msssim: msssim_u8 / msssim_u16 beside ssim_u8 / ssim_u16 on one chunk
of correlated 1080 x 1920 pairs, from events; then evaluate_sequence (with --yuv: evaluate_yuv) with metrics only, ``msssim`` off and
on in alternating passes of one process.  (Against another commit there is no switch: export that commit into a directory of its own,
build it there, and run this tool, or a pass set of evaluate_yuv, from each tree in fresh processes in alternation on one box; DESIGN.md
section 5.000000000 has the figures taken that way.)  --niqe PARAMS (a pristine model, `metrics.niqe_params`): the seven launches of
`niqe_features_u8` beside ssim_u8 and msssim_u8 on one chunk of 1080 x 1920 frames in alternating passes, and each of its kernels
alone, from events; then the evaluator with metrics only, ``niqe`` off and on in alternating passes of one process.  --brisque MODEL
(a support-vector model, `metrics.brisque_params`): the seven launches of `brisque_features_u8` beside ssim_u8 (and, with --niqe
PARAMS, `niqe_features_u8`) on the same chunk, each of its kernels alone, and the evaluator with ``brisque`` off and on.  --tof:
the launches of `tof_frames_u8` on the same chunk (2 K Farneback pairs, the scratch held) beside ssim_u8 (and, with --niqe PARAMS,
`niqe_features_u8`), each kernel's share summed over the stages, and the evaluator with ``tof`` off and on.  --lpips MODEL (a model
file, `metrics.lpips_params`; ``random``: He-initialised weights of the published widths, which cost what real ones cost): the
launches of `lpips_layers_u8` on the same chunk (K pairs through the trunk one pair per pass, the scratch held) beside ssim_u8, the
split per stage -- stem, the convolutions of each stage, the pools, the distances, the fold -- from events round every launch, and
the evaluator with ``lpips`` off and on; --only kernels / --only evaluator runs one half.  --rescale-metrics (with --pix-fmt NAME above
8 bits; it is looked for first, so the options it shares keep their meaning): the six 16-bit sample kernels against their 8-bit twins
on one chunk of 1080 x 1920 frames, the two forms in alternating passes, medians of five from events (tOF's level images summed over
the stages); then evaluate_yuv at NAME with ``rescale_metrics=True``, each of the given options off and on in alternating passes."""
import os
import sys
import tempfile
import time

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


def yuv():
    import time
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd import kernels as K
    from cdfo_amd.evaluate import evaluate_sequence, evaluate_yuv, write_synthetic_sequence, write_synthetic_sequence_yuv
    from cdfo_amd.priors import load_priors, load_sequence
    from cdfo_amd.streaming import StreamingSR
    T, H, W = _arg("--size", 3, [64, 270, 480])
    chunk, reps = _arg("--chunk", 1, 8), _arg("--repeats", 1, 5)
    model = CVSR_V8().cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        lr, side, gt = write_synthetic_sequence(os.path.join(tmp, "png"), T, H, W)
        lr_yuv, side_yuv, gt_yuv = write_synthetic_sequence_yuv(os.path.join(tmp, "raw"), T, H, W)
        seq = load_sequence(lr, side)
        s = StreamingSR(model, seq["lr"], seq["pms"], seq["rms"], seq["ufs"], seq["mvl0"], seq["mvl1"])
        s.run_chunked(chunk)
        fps = []
        for _ in range(reps):
            s.run_chunked(chunk)
            fps.append(s.fps)
        base = float(np.median(fps))
        print(f"run_chunked(chunk={chunk}) alone, {T} frames {H}x{W}: frames/s per pass {' '.join('%.2f' % f for f in fps)}; median "
              f"{base:.2f}", flush=True)
        del s, seq
        secs = []
        for _ in range(reps):
            t0 = time.perf_counter()
            load_priors(side, T)
            secs.append(time.perf_counter() - t0)
        priors = float(np.median(secs))
        print(f"load_priors ({2 * (T - 1)} LR-sized PNGs, {3 * (T - 1)} NPYs), before the first chunk of either path: median "
              f"{priors * 1e3:.1f} ms", flush=True)
        png_out, yuv_out = os.path.join(tmp, "out"), os.path.join(tmp, "out.yuv")
        runs = (("evaluate_sequence, metrics only", lambda: evaluate_sequence(model, lr, side, gt_dir=gt, chunk=chunk)),
                ("evaluate_yuv, metrics only", lambda: evaluate_yuv(model, lr_yuv, W, H, side_yuv, gt_yuv=gt_yuv, chunk=chunk)),
                ("evaluate_sequence, metrics + PNGs, 8 workers",
                 lambda: evaluate_sequence(model, lr, side, gt_dir=gt, save_dir=png_out, chunk=chunk)),
                ("evaluate_yuv, metrics + I420 file",
                 lambda: evaluate_yuv(model, lr_yuv, W, H, side_yuv, gt_yuv=gt_yuv, save_yuv=yuv_out, chunk=chunk)))
        for label, run in runs:
            run()
            rs = [run() for _ in range(reps)]
            fwd, tot = [r.frames / r.seconds_forward for r in rs], [r.frames / r.seconds_total for r in rs]
            sec = float(np.median([r.seconds_total for r in rs]))
            print(f"{label}: forward-only frames/s median {np.median(fwd):.2f}; end to end (files read included) per pass "
                  f"{' '.join('%.2f' % f for f in tot)}; median {np.median(tot):.2f} ({np.median(tot) / base:.3f} of run_chunked alone); "
                  f"{sec:.3f} s per pass, of which load_priors {100 * priors / sec:.1f} %", flush=True)
        # chroma_up4 on one chunk's worth of planes (2 per frame), with and without ground truth, from events
        hc, wc = H // 2, W // 2
        src = torch.randint(0, 256, (2 * chunk, hc, wc), dtype=torch.uint8).cuda()
        gt8 = torch.randint(0, 256, (2 * chunk, 4 * hc, 4 * wc), dtype=torch.uint8).cuda()
        dst, _ = K.chroma_up4(src, gt=gt8)
        with_gt, _ = _median_ms(lambda: K.chroma_up4(src, gt=gt8, dst=dst))
        plain, _ = _median_ms(lambda: K.chroma_up4(src, dst=dst))
        mb = 2 * chunk * hc * wc / 1e6
        print(f"chroma_up4 per chunk of {chunk} frames ({2 * chunk} planes {hc}x{wc} -> {4 * hc}x{4 * wc}; wrapper included), median of "
              f"5: {plain:.3f} ms ({17 * mb / plain:.1f} GB/s), with the squared-difference sum {with_gt:.3f} ms "
              f"({33 * mb / with_gt:.1f} GB/s)", flush=True)


def pix_fmt():
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    from cdfo_amd.evaluate import evaluate_yuv, write_synthetic_sequence_yuv
    from cdfo_amd.yuv import parse_pix_fmt
    fmt = parse_pix_fmt(sys.argv[sys.argv.index("--pix-fmt") + 1])
    T, H, W = _arg("--size", 3, [64, 270, 480])
    chunk, reps = _arg("--chunk", 1, 8), _arg("--repeats", 1, 5)
    model = CVSR_V8().cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        base = None
        for name in ("yuv420p", fmt.name):
            lr, side, gt = write_synthetic_sequence_yuv(os.path.join(tmp, name), T, H, W, pix_fmt=name)
            out = os.path.join(tmp, name + ".yuv")
            run = lambda: evaluate_yuv(model, lr, W, H, side, gt_yuv=gt, save_yuv=out, chunk=chunk, pix_fmt=name)
            run()
            rs = [run() for _ in range(reps)]
            tot, fwd = [r.frames / r.seconds_total for r in rs], [r.frames / r.seconds_forward for r in rs]
            med = float(np.median(tot))
            base = med if base is None else base
            print(f"evaluate_yuv, {name}, metrics + file, {T} frames {H}x{W}, chunk {chunk}: forward-only frames/s median "
                  f"{np.median(fwd):.2f}; end to end per pass {' '.join('%.2f' % f for f in tot)}; median {med:.2f} (spread "
                  f"{100 * (max(tot) - min(tot)) / med:.2f} %; {med / base:.4f} of the 8-bit run)", flush=True)
    if fmt.sample_bytes == 1:
        return
    # the three kernels and their 8-bit twins on one chunk of 1080 x 1920 frames (270 x 480 LR), from events
    h, w, peak = 270, 480, fmt.peak
    src = torch.rand((chunk, 1, 4 * ((h + 7) // 8 * 8), 4 * w), device="cuda") * 1.2 - 0.1
    frames = lambda n, hh, ww, top, kind: torch.from_numpy(
        np.random.RandomState(n + hh).randint(0, top + 1, (n, hh, ww)).astype(kind)).cuda()
    gt8, gt16 = frames(chunk, 4 * h, 4 * w, 255, np.uint8), frames(chunk, 4 * h, 4 * w, peak, np.uint16)
    c8, c16 = frames(2 * chunk, h // 2, w // 2, 255, np.uint8), frames(2 * chunk, h // 2, w // 2, peak, np.uint16)
    gc8, gc16 = frames(2 * chunk, 2 * h, 2 * w, 255, np.uint8), frames(2 * chunk, 2 * h, 2 * w, peak, np.uint16)
    y8, _ = K.finish_frames(src, h, w, gt=gt8)
    y16, _ = K.finish_frames(src, h, w, gt=gt16, peak=peak)
    d8, _ = K.chroma_up4(c8, gt=gc8)
    d16, _ = K.chroma_up4(c16, gt=gc16, peak=peak)
    pairs = (("finish_frames with the squared-difference sum", "8/6", lambda: K.finish_frames(src, h, w, gt=gt8, dst=y8),
              lambda: K.finish_frames(src, h, w, gt=gt16, dst=y16, peak=peak)),
             ("chroma_up4 with the squared-difference sum", "2", lambda: K.chroma_up4(c8, gt=gc8, dst=d8),
              lambda: K.chroma_up4(c16, gt=gc16, dst=d16, peak=peak)),
             ("SSIM", "about 1 (fp64 compute)", lambda: M.ssim_u8(y8, gt8, 4), lambda: M.ssim_u16(y16, gt16, 4, peak)))
    for label, ratio, f8, f16 in pairs:
        (m8, a8), (m16, a16) = _median_ms(f8), _median_ms(f16)
        print(f"{label}, chunk of {chunk} frames 1080x1920 (wrapper included), median of 5: 8-bit {m8:.3f} ms (passes "
              f"{' '.join('%.3f' % x for x in a8)}), 16-bit at peak {peak} {m16:.3f} ms (passes {' '.join('%.3f' % x for x in a16)}): "
              f"x{m16 / m8:.3f}, byte ratio {ratio}", flush=True)


def msssim():
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd import metrics as M
    from cdfo_amd.evaluate import evaluate_sequence, evaluate_yuv, write_synthetic_sequence, write_synthetic_sequence_yuv
    T, H, W = _arg("--size", 3, [64, 270, 480])
    chunk, reps = _arg("--chunk", 1, 8), _arg("--repeats", 1, 5)
    rs = np.random.RandomState(0)
    for peak, kind, sigma in ((255, np.uint8, 20), (1023, np.uint16, 80)):
        a = rs.randint(0, peak + 1, (chunk, 4 * H, 4 * W))
        b = np.clip(a + np.rint(sigma * rs.randn(*a.shape)).astype(np.int64), 0, peak)
        a, b = torch.from_numpy(a.astype(kind)).cuda(), torch.from_numpy(b.astype(kind)).cuda()
        one, many = (M.ssim_u8, M.msssim_u8) if peak == 255 else (lambda *x: M.ssim_u16(*x, peak), lambda *x: M.msssim_u16(*x, peak))
        scratch = M.msssim_scratch(chunk, *M.msssim_region(4 * H, 4 * W, 4 * H, 4 * W, 4), a.device)
        (ss, ps), (ms, pm) = _median_ms(lambda: one(a, b, 4)), _median_ms(lambda: many(a, b, 4))
        mc, pc = _median_ms(lambda: M.msssim_components(a, b, 4, None if peak == 255 else peak, scratch))
        print(f"chunk of {chunk} pairs {4 * H}x{4 * W}, peak {peak}, crop 4 (wrapper included), median of 5: SSIM {ss:.3f} ms (passes "
              f"{' '.join('%.3f' % x for x in ps)}); MS-SSIM {ms:.3f} ms (passes {' '.join('%.3f' % x for x in pm)}): x{ms / ss:.3f}; "
              f"its ten means alone, as the evaluators call it (scratch held, no host combine) {mc:.3f} ms (passes "
              f"{' '.join('%.3f' % x for x in pc)}): x{mc / ss:.3f}", flush=True)
    model = CVSR_V8().cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        if "--yuv" in sys.argv:
            lr, side, gt = write_synthetic_sequence_yuv(tmp, T, H, W)
            run = lambda on: evaluate_yuv(model, lr, W, H, side, gt_yuv=gt, chunk=chunk, msssim=on)
        else:
            lr, side, gt = write_synthetic_sequence(tmp, T, H, W)
            run = lambda on: evaluate_sequence(model, lr, side, gt_dir=gt, chunk=chunk, msssim=on)
        run(False), run(True)
        fps = {False: [], True: []}
        for _ in range(reps):                                # alternating passes: drift of the box falls on both alike
            for on in (False, True):
                r = run(on)
                fps[on].append(r.frames / r.seconds_total)
        off, on = float(np.median(fps[False])), float(np.median(fps[True]))
        print(f"{'evaluate_yuv' if '--yuv' in sys.argv else 'evaluate_sequence'}, metrics only, {T} frames {H}x{W}, chunk {chunk}, end to "
              f"end frames/s: msssim off per pass {' '.join('%.2f' % f for f in fps[False])}; median {off:.2f}; msssim on per pass "
              f"{' '.join('%.2f' % f for f in fps[True])}; median {on:.2f} ({on / off:.4f} of off)", flush=True)


def niqe():
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    from cdfo_amd.evaluate import evaluate_sequence, evaluate_yuv, write_synthetic_sequence, write_synthetic_sequence_yuv
    params = M.niqe_params(sys.argv[sys.argv.index("--niqe") + 1])
    T, H, W = _arg("--size", 3, [64, 270, 480])
    chunk, reps = _arg("--chunk", 1, 8), _arg("--repeats", 1, 5)
    rs = np.random.RandomState(0)
    a = rs.randint(0, 256, (chunk, 4 * H, 4 * W))
    b = np.clip(a + np.rint(20 * rs.randn(*a.shape)).astype(np.int64), 0, 255)
    a, b = torch.from_numpy(a.astype(np.uint8)).cuda(), torch.from_numpy(b.astype(np.uint8)).cuda()
    R, Cc = M.niqe_region(4 * H, 4 * W)
    nq, ms = M.niqe_scratch(chunk, R, Cc, a.device), M.msssim_scratch(chunk, *M.msssim_region(4 * H, 4 * W, 4 * H, 4 * W, 4), a.device)
    forms = (("ssim_u8", lambda: M.ssim_u8(a, b, 4)), ("msssim_components", lambda: M.msssim_components(a, b, 4, None, ms)),
             ("niqe_features_u8", lambda: M.niqe_features_u8(a, nq)))
    times = {name: [] for name, _ in forms}
    for name, fn in forms:
        fn()
    torch.cuda.synchronize()
    for _ in range(5):                                       # alternating forms: drift of the box falls on all alike
        for name, fn in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    med = {name: float(np.median(v)) for name, v in times.items()}
    print(f"chunk of {chunk} frames {4 * H}x{4 * W} (NIQE region {R}x{Cc}; wrappers included, scratch held), median of 5 alternating passes: "
          + "; ".join(f"{name} {med[name]:.3f} ms (passes {' '.join('%.3f' % x for x in times[name])})" for name, _ in forms)
          + f": NIQE's features x{med['niqe_features_u8'] / med['ssim_u8']:.2f} of SSIM, x{med['niqe_features_u8'] / med['msssim_components']:.2f} "
          f"of MS-SSIM's means, {med['niqe_features_u8'] / chunk:.3f} ms per frame", flush=True)
    win, table = M.niqe_window(), M._niqe_table_on(a.device)
    m1, hf = K.niqe_mscn(a, R, Cc, win), K.niqe_half(a, R, Cc)
    m2 = K.niqe_mscn(hf, R // 2, Cc // 2, win)
    s1, s2 = K.niqe_block_sums(m1, 96), K.niqe_block_sums(m2, 48)
    out = torch.empty((chunk, s1.shape[1], 36), dtype=torch.float64, device=a.device)
    split = (("mscn_u8", lambda: K.niqe_mscn(a, R, Cc, win, m1)), ("half", lambda: K.niqe_half(a, R, Cc, hf)),
             ("mscn_f64", lambda: K.niqe_mscn(hf, R // 2, Cc // 2, win, m2)), ("block_sums 96", lambda: K.niqe_block_sums(m1, 96, s1)),
             ("block_sums 48", lambda: K.niqe_block_sums(m2, 48, s2)), ("features x2", lambda: (K.niqe_features(s1, 9216, table, 0, out),
                                                                                              K.niqe_features(s2, 2304, table, 1, out))))
    print("the split, median of 5 each (wrapper included): " + "; ".join(f"{name} {_median_ms(fn)[0]:.3f} ms" for name, fn in split), flush=True)
    t0 = time.perf_counter()
    scores = M.niqe_from_features(out, params)
    print(f"niqe_from_features on the host, {chunk} frames of {s1.shape[1]} blocks: {(time.perf_counter() - t0) * 1e3:.2f} ms "
          f"(scores of the noise frames {scores.min():.2f} .. {scores.max():.2f})", flush=True)
    model = CVSR_V8().cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        if "--yuv" in sys.argv:
            lr, side, gt = write_synthetic_sequence_yuv(tmp, T, H, W)
            run = lambda on: evaluate_yuv(model, lr, W, H, side, gt_yuv=gt, chunk=chunk, niqe=params if on else None)
        else:
            lr, side, gt = write_synthetic_sequence(tmp, T, H, W)
            run = lambda on: evaluate_sequence(model, lr, side, gt_dir=gt, chunk=chunk, niqe=params if on else None)
        run(False), run(True)
        fps = {False: [], True: []}
        for _ in range(reps):                                # alternating passes: drift of the box falls on both alike
            for on in (False, True):
                r = run(on)
                fps[on].append(r.frames / r.seconds_total)
        off, on = float(np.median(fps[False])), float(np.median(fps[True]))
        print(f"{'evaluate_yuv' if '--yuv' in sys.argv else 'evaluate_sequence'}, metrics only, {T} frames {H}x{W}, chunk {chunk}, end to "
              f"end frames/s: niqe off per pass {' '.join('%.2f' % f for f in fps[False])}; median {off:.2f}; niqe on per pass "
              f"{' '.join('%.2f' % f for f in fps[True])}; median {on:.2f} ({on / off:.4f} of off)", flush=True)


def brisque():
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    from cdfo_amd.evaluate import evaluate_sequence, evaluate_yuv, write_synthetic_sequence, write_synthetic_sequence_yuv
    params = M.brisque_params(sys.argv[sys.argv.index("--brisque") + 1])
    T, H, W = _arg("--size", 3, [64, 270, 480])
    chunk, reps = _arg("--chunk", 1, 8), _arg("--repeats", 1, 5)
    rs = np.random.RandomState(0)
    a = rs.randint(0, 256, (chunk, 4 * H, 4 * W))
    b = np.clip(a + np.rint(20 * rs.randn(*a.shape)).astype(np.int64), 0, 255)
    a, b = torch.from_numpy(a.astype(np.uint8)).cuda(), torch.from_numpy(b.astype(np.uint8)).cuda()
    bq = M.brisque_scratch(chunk, 4 * H, 4 * W, a.device)
    forms = [("ssim_u8", lambda: M.ssim_u8(a, b, 4)), ("brisque_features_u8", lambda: M.brisque_features_u8(a, bq))]
    if "--niqe" in sys.argv:
        nq = M.niqe_scratch(chunk, *M.niqe_region(4 * H, 4 * W), a.device)
        forms.insert(1, ("niqe_features_u8", lambda: M.niqe_features_u8(a, nq)))
    times = {name: [] for name, _ in forms}
    for name, fn in forms:
        fn()
    torch.cuda.synchronize()
    for _ in range(5):                                       # alternating forms: drift of the box falls on all alike
        for name, fn in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    med = {name: float(np.median(v)) for name, v in times.items()}
    print(f"chunk of {chunk} frames {4 * H}x{4 * W} (wrappers included, scratch held), median of 5 alternating passes: "
          + "; ".join(f"{name} {med[name]:.3f} ms (passes {' '.join('%.3f' % x for x in times[name])})" for name, _ in forms)
          + f": BRISQUE's features x{med['brisque_features_u8'] / med['ssim_u8']:.2f} of SSIM, {med['brisque_features_u8'] / chunk:.3f} ms "
          "per frame", flush=True)
    win, table = M.brisque_window(), M._brisque_table_on(a.device)
    m1, hf = K.brisque_mscn(a, win), K.brisque_half(a)
    m2 = K.brisque_mscn(hf, win)
    s1, s2 = K.brisque_sums(m1), K.brisque_sums(m2)
    out = torch.empty((chunk, 36), dtype=torch.float64, device=a.device)
    n1, n2 = m1.shape[1] * m1.shape[2], m2.shape[1] * m2.shape[2]
    split = (("mscn_u8", lambda: K.brisque_mscn(a, win, m1)), ("half", lambda: K.brisque_half(a, hf)),
             ("mscn_f64", lambda: K.brisque_mscn(hf, win, m2)), ("sums scale 1", lambda: K.brisque_sums(m1, s1)),
             ("sums scale 2", lambda: K.brisque_sums(m2, s2)), ("features x2", lambda: (K.brisque_features(s1, n1, table, 0, out),
                                                                                       K.brisque_features(s2, n2, table, 1, out))))
    print("the split, median of 5 each (wrapper included): " + "; ".join(f"{name} {_median_ms(fn)[0]:.3f} ms" for name, fn in split), flush=True)
    t0 = time.perf_counter()
    scores = M.brisque_from_features(out, params)
    print(f"brisque_from_features on the host, {chunk} frames, {len(params.sv)} support vectors: {(time.perf_counter() - t0) * 1e3:.2f} ms "
          f"(scores of the noise frames {scores.min():.2f} .. {scores.max():.2f})", flush=True)
    model = CVSR_V8().cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        if "--yuv" in sys.argv:
            lr, side, gt = write_synthetic_sequence_yuv(tmp, T, H, W)
            run = lambda on: evaluate_yuv(model, lr, W, H, side, gt_yuv=gt, chunk=chunk, brisque=params if on else None)
        else:
            lr, side, gt = write_synthetic_sequence(tmp, T, H, W)
            run = lambda on: evaluate_sequence(model, lr, side, gt_dir=gt, chunk=chunk, brisque=params if on else None)
        run(False), run(True)
        fps = {False: [], True: []}
        for _ in range(reps):                                # alternating passes: drift of the box falls on both alike
            for on in (False, True):
                r = run(on)
                fps[on].append(r.frames / r.seconds_total)
        off, on = float(np.median(fps[False])), float(np.median(fps[True]))
        print(f"{'evaluate_yuv' if '--yuv' in sys.argv else 'evaluate_sequence'}, metrics only, {T} frames {H}x{W}, chunk {chunk}, end to "
              f"end frames/s: brisque off per pass {' '.join('%.2f' % f for f in fps[False])}; median {off:.2f}; brisque on per pass "
              f"{' '.join('%.2f' % f for f in fps[True])}; median {on:.2f} ({on / off:.4f} of off)", flush=True)


def tof():
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    from cdfo_amd.evaluate import evaluate_sequence, evaluate_yuv, write_synthetic_sequence, write_synthetic_sequence_yuv
    T, H, W = _arg("--size", 3, [64, 270, 480])
    chunk, reps = _arg("--chunk", 1, 8), _arg("--repeats", 1, 5)
    rs = np.random.RandomState(0)
    a = rs.randint(0, 256, (chunk, 4 * H, 4 * W))
    b = np.clip(a + np.rint(20 * rs.randn(*a.shape)).astype(np.int64), 0, 255)
    a, b = torch.from_numpy(a.astype(np.uint8)).cuda(), torch.from_numpy(b.astype(np.uint8)).cuda()
    ts = M.tof_scratch(2 * chunk, 4 * H, 4 * W, a.device)
    forms = [("ssim_u8", lambda: M.ssim_u8(a, b, 4)), ("tof_frames_u8", lambda: M.tof_frames_u8(a, b, a[0], b[0], ts))]
    if "--niqe" in sys.argv:
        params = M.niqe_params(sys.argv[sys.argv.index("--niqe") + 1])
        nq = M.niqe_scratch(chunk, *M.niqe_region(4 * H, 4 * W), a.device)
        forms.insert(1, ("niqe_features_u8", lambda: M.niqe_features_u8(a, nq)))
    times = {name: [] for name, _ in forms}
    for name, fn in forms:
        fn()
    torch.cuda.synchronize()
    for _ in range(5):                                       # alternating forms: drift of the box falls on all alike
        for name, fn in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    med = {name: float(np.median(v)) for name, v in times.items()}
    stages = M.tof_size(4 * H, 4 * W)
    print(f"chunk of {chunk} frames {4 * H}x{4 * W} = {2 * chunk} pairs, {len(stages)} stages (wrappers included, scratch of {ts.nbytes} bytes "
          "held), median of 5 alternating passes: "
          + "; ".join(f"{name} {med[name]:.3f} ms (passes {' '.join('%.3f' % x for x in times[name])})" for name, _ in forms)
          + f": tOF x{med['tof_frames_u8'] / med['ssim_u8']:.1f} of SSIM, {med['tof_frames_u8'] / chunk:.3f} ms per frame", flush=True)
    # the split: each kernel on the chunk's 2 K pairs, summed over the stages it runs at (and the times it runs there)
    N, kern = 2 * chunk, M.tof_poly_kernels()
    split = {"level_u8 x2": 0.0, "polyexp": 0.0, "flow_up": 0.0, "matrices x3": 0.0, "blur_solve x3": 0.0}
    prev = None
    for k, h, w in stages:
        img = torch.empty((N, 2, h, w), dtype=torch.float64, device=a.device)
        level = lambda: (K.tof_level(a, a, h, w, M.tof_taps(k), first=a[0], out=img[:chunk]),
                         K.tof_level(b, b, h, w, M.tof_taps(k), first=b[0], out=img[chunk:]))
        split["level_u8 x2"] += _median_ms(level)[0]
        R = K.tof_polyexp(img, kern)
        split["polyexp"] += _median_ms(lambda: K.tof_polyexp(img, kern, R))[0]
        flow = None
        if prev is not None:
            flow = K.tof_flow_up(prev, h, w)
            split["flow_up"] += _median_ms(lambda: K.tof_flow_up(prev, h, w, flow))[0]
        Mx = K.tof_matrices(R, flow)
        split["matrices x3"] += 3 * _median_ms(lambda: K.tof_matrices(R, flow, Mx))[0]
        prev = K.tof_blur_solve(Mx)
        split["blur_solve x3"] += 3 * _median_ms(lambda: K.tof_blur_solve(Mx, prev))[0]
        del img, R, Mx
    split["epe"] = _median_ms(lambda: K.tof_epe(prev[:chunk], prev[chunk:]))[0]
    del prev
    print("the split over all stages, medians of 5 each (wrapper included): " + "; ".join(f"{n} {v:.3f} ms" for n, v in split.items())
          + f"; sum {sum(split.values()):.3f} ms", flush=True)
    model = CVSR_V8().cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        if "--yuv" in sys.argv:
            lr, side, gt = write_synthetic_sequence_yuv(tmp, T, H, W)
            run = lambda on: evaluate_yuv(model, lr, W, H, side, gt_yuv=gt, chunk=chunk, tof=on)
        else:
            lr, side, gt = write_synthetic_sequence(tmp, T, H, W)
            run = lambda on: evaluate_sequence(model, lr, side, gt_dir=gt, chunk=chunk, tof=on)
        run(False), run(True)
        fps = {False: [], True: []}
        for _ in range(reps):                                # alternating passes: drift of the box falls on both alike
            for on in (False, True):
                r = run(on)
                fps[on].append(r.frames / r.seconds_total)
        off, on = float(np.median(fps[False])), float(np.median(fps[True]))
        print(f"{'evaluate_yuv' if '--yuv' in sys.argv else 'evaluate_sequence'}, metrics only, {T} frames {H}x{W}, chunk {chunk}, end to "
              f"end frames/s: tof off per pass {' '.join('%.2f' % f for f in fps[False])}; median {off:.2f}; tof on per pass "
              f"{' '.join('%.2f' % f for f in fps[True])}; median {on:.2f} ({on / off:.4f} of off); mean tOF {r.mean_tof:.5f}", flush=True)


def lpips():
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    from cdfo_amd.evaluate import evaluate_sequence, evaluate_yuv, write_synthetic_sequence, write_synthetic_sequence_yuv
    source = sys.argv[sys.argv.index("--lpips") + 1]
    params = M.lpips_random_params() if source == "random" else M.lpips_params(source)
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    T, H, W = _arg("--size", 3, [64, 270, 480])
    chunk, reps = _arg("--chunk", 1, 8), _arg("--repeats", 1, 5)
    if only != "evaluator":
        rs = np.random.RandomState(0)
        a = rs.randint(0, 256, (chunk, 4 * H, 4 * W))
        b = np.clip(a + np.rint(20 * rs.randn(*a.shape)).astype(np.int64), 0, 255)
        a, b = torch.from_numpy(a.astype(np.uint8)).cuda(), torch.from_numpy(b.astype(np.uint8)).cuda()
        ls = M.lpips_scratch(chunk, 4 * H, 4 * W, params, a.device)
        forms = [("ssim_u8", lambda: M.ssim_u8(a, b, 4)), ("lpips_layers_u8", lambda: M.lpips_layers_u8(a, b, params, ls))]
        times = {name: [] for name, _ in forms}
        for name, fn in forms:
            fn()
        torch.cuda.synchronize()
        for _ in range(5):                                   # alternating forms: drift of the box falls on all alike
            for name, fn in forms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
        med = {name: float(np.median(v)) for name, v in times.items()}
        print(f"chunk of {chunk} pairs {4 * H}x{4 * W}, widths {params.widths} (wrappers included, scratch of {ls.nbytes} bytes held, "
              f"{ls.pairs} pair per pass), median of 5 alternating passes: "
              + "; ".join(f"{name} {med[name]:.3f} ms (passes {' '.join('%.3f' % x for x in times[name])})" for name, _ in forms)
              + f": LPIPS x{med['lpips_layers_u8'] / med['ssim_u8']:.0f} of SSIM, {med['lpips_layers_u8'] / chunk:.3f} ms per pair", flush=True)
        # the split: `lpips_layers_u8`'s own launches with events round each, summed per kind over the chunk's passes
        m, sizes, widths = M._lpips_on(params, a.device), ls.sizes, params.widths
        first = [chunk * sum(ls.strips[:k]) for k in range(5)]
        partials = ls.partials[:chunk * sum(ls.strips)]

        def one_chunk():
            marks = []

            def timed(label, fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn()
                e1.record()
                marks.append((label, e0, e1))
                return out

            for j in range(chunk):
                act = lambda buf, k, c: buf[:2 * sizes[k][0] * sizes[k][1] * c].view(2, sizes[k][0], sizes[k][1], c)
                cur, other = ls.a, ls.b
                x = act(cur, 0, widths[0])
                timed("stem x2", lambda: (K.lpips_stem(a[j:j + 1], m.w0, m.b0, True, out=x[:1]), K.lpips_stem(b[j:j + 1], m.w0, m.b0, True, out=x[1:])))
                i = 0
                for k, convs in enumerate(M.LPIPS_STAGES):
                    if k:
                        x = timed("pools", lambda: K.lpips_pool2(x, act(other, k, widths[k - 1])))
                        cur, other = other, cur
                    for _ in range(convs - (k == 0)):
                        x = timed(f"convs stage {k + 1}", lambda: K.conv(x, m.convs[i], pad=1, act=K.ACT_RELU, prec=K.PREC_F32,
                                                                          out=act(other, k, widths[k])))
                        cur, other = other, cur
                        i += 1
                    timed("dist", lambda: K.lpips_dist(x[:1], x[1:], m.lins[k],
                                                       partials[first[k]:first[k] + chunk * ls.strips[k]].view(chunk, ls.strips[k])[j:j + 1]))
            timed("fold", lambda: K.lpips_fold(partials, chunk, ls.strips, [hk * wk for hk, wk in sizes]))
            torch.cuda.synchronize()
            sums = {}
            for label, e0, e1 in marks:
                sums[label] = sums.get(label, 0.0) + e0.elapsed_time(e1)
            return sums

        one_chunk()
        passes = [one_chunk() for _ in range(5)]
        split = {label: float(np.median([p[label] for p in passes])) for label in passes[0]}
        flop = 2.0 * 9 * sum(w.shape[0] * w.shape[1] * sizes[k][0] * sizes[k][1]
                             for k, n in enumerate(M.LPIPS_STAGES) for w in params.weights[sum(M.LPIPS_STAGES[:k]):sum(M.LPIPS_STAGES[:k]) + n])
        conv_ms = sum(v for n, v in split.items() if n.startswith("convs") or n.startswith("stem"))
        print(f"the split over the chunk's {chunk} passes, medians of 5 (wrapper included): " + "; ".join(f"{n} {v:.3f} ms" for n, v in split.items())
              + f"; sum {sum(split.values()):.3f} ms; the trunk is {2 * flop / 1e12:.3f} TFLOP per pair: {2 * flop * chunk / conv_ms / 1e9:.1f} TFLOP/s "
              "over the stem and the convolutions", flush=True)
        del a, b, ls, partials
    if only == "kernels":
        return
    model = CVSR_V8().cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        if "--yuv" in sys.argv:
            lr, side, gt = write_synthetic_sequence_yuv(tmp, T, H, W)
            run = lambda on: evaluate_yuv(model, lr, W, H, side, gt_yuv=gt, chunk=chunk, lpips=params if on else None)
        else:
            lr, side, gt = write_synthetic_sequence(tmp, T, H, W)
            run = lambda on: evaluate_sequence(model, lr, side, gt_dir=gt, chunk=chunk, lpips=params if on else None)
        run(False), run(True)
        fps = {False: [], True: []}
        for _ in range(reps):                                # alternating passes: drift of the box falls on both alike
            for on in (False, True):
                r = run(on)
                fps[on].append(r.frames / r.seconds_total)
        off, on = float(np.median(fps[False])), float(np.median(fps[True]))
        print(f"{'evaluate_yuv' if '--yuv' in sys.argv else 'evaluate_sequence'}, metrics only, {T} frames {H}x{W}, chunk {chunk}, end to "
              f"end frames/s: lpips off per pass {' '.join('%.2f' % f for f in fps[False])}; median {off:.2f}; lpips on per pass "
              f"{' '.join('%.2f' % f for f in fps[True])}; median {on:.2f} ({on / off:.4f} of off); mean LPIPS {r.mean_lpips:.5f}", flush=True)


def rescale_metrics():
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    from cdfo_amd.evaluate import evaluate_yuv, write_synthetic_sequence_yuv
    from cdfo_amd.yuv import parse_pix_fmt
    fmt = parse_pix_fmt(sys.argv[sys.argv.index("--pix-fmt") + 1] if "--pix-fmt" in sys.argv else "yuv420p10le")
    if fmt.sample_bytes == 1:
        sys.exit("--rescale-metrics measures a format above 8 bits: give --pix-fmt one")
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    T, H, W = _arg("--size", 3, [64, 270, 480])
    chunk, reps, peak = _arg("--chunk", 1, 8), _arg("--repeats", 1, 5), fmt.peak
    value = lambda name: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None
    lp = value("--lpips")
    lp = None if lp is None else M.lpips_random_params() if lp == "random" else M.lpips_params(lp)
    if only != "evaluator":
        # the six sample kernels against their 8-bit twins on one chunk of 1080 x 1920 frames, the two forms in alternating passes
        h, w = 1080, 1920
        rs = np.random.RandomState(0)
        a8 = torch.from_numpy(rs.randint(0, 256, (chunk, h, w)).astype(np.uint8)).cuda()
        a16 = torch.from_numpy(rs.randint(0, peak + 1, (chunk, h, w)).astype(np.uint16)).cuda()
        R, Cc = M.niqe_region(h, w)
        nwin, bwin = M.niqe_window(), M.brisque_window()
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
        nm, nh, bm, bh = f64(chunk, R, Cc), f64(chunk, R // 2, Cc // 2), f64(chunk, h, w), f64(chunk, (h + 1) // 2, (w + 1) // 2)
        m = M._lpips_on(lp or M.lpips_random_params(), a8.device)
        stem = torch.empty((chunk, h, w, m.w0.shape[0]), dtype=torch.float32, device="cuda")
        levels = [(k, hh, ww, f64(chunk, 2, hh, ww)) for k, hh, ww in M.tof_size(h, w)]

        def level(a, p):
            for k, hh, ww, img in levels:
                K.tof_level(a, a, hh, ww, M.tof_taps(k), first=a[0], out=img, peak=p)

        pairs = (("niqe_mscn", "9/10", lambda a, p: K.niqe_mscn(a, R, Cc, nwin, nm, peak=p)),
                 ("niqe_half", "3/4", lambda a, p: K.niqe_half(a, R, Cc, nh, peak=p)),
                 ("brisque_mscn", "9/10", lambda a, p: K.brisque_mscn(a, bwin, bm, peak=p)),
                 ("brisque_half", "3/4", lambda a, p: K.brisque_half(a, bh, peak=p)),
                 (f"tof_level, {len(levels)} stages", "compute", level),
                 (f"lpips_stem, C0 {m.w0.shape[0]}", f"{4 * m.w0.shape[0] + 1}/{4 * m.w0.shape[0] + 2}",
                  lambda a, p: K.lpips_stem(a, m.w0, m.b0, True, out=stem, peak=p)))
        for label, ratio, fn in pairs:
            forms = ((8, lambda: fn(a8, None)), (16, lambda: fn(a16, peak)))
            times = {8: [], 16: []}
            for _, run in forms:
                run()
            torch.cuda.synchronize()
            for _ in range(5):                                   # alternating forms: drift of the box falls on both alike
                for bits, run in forms:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run()
                    e1.record()
                    torch.cuda.synchronize()
                    times[bits].append(e0.elapsed_time(e1))
            m8, m16 = float(np.median(times[8])), float(np.median(times[16]))
            print(f"{label}, chunk of {chunk} frames {h}x{w} (wrapper included), median of 5 alternating passes: 8-bit {m8:.3f} ms (passes "
                  f"{' '.join('%.3f' % x for x in times[8])}), 16-bit at peak {peak} {m16:.3f} ms (passes "
                  f"{' '.join('%.3f' % x for x in times[16])}): x{m16 / m8:.3f}, byte ratio 8-bit/16-bit {ratio}", flush=True)
        del a8, a16, nm, nh, bm, bh, stem, levels
    if only == "kernels":
        return
    options = [(name, dict({name: v})) for name, v in (("niqe", value("--niqe")), ("brisque", value("--brisque")), ("tof", "--tof" in sys.argv or None),
                                                       ("lpips", lp)) if v]
    model = CVSR_V8().cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        lr, side, gt = write_synthetic_sequence_yuv(tmp, T, H, W, pix_fmt=fmt.name)
        for name, kw in options:
            run = lambda on: evaluate_yuv(model, lr, W, H, side, gt_yuv=gt, chunk=chunk, pix_fmt=fmt.name, rescale_metrics=True,
                                          **(kw if on else {}))
            run(False), run(True)
            fps = {False: [], True: []}
            for _ in range(reps):                                # alternating passes: drift of the box falls on both alike
                for on in (False, True):
                    r = run(on)
                    fps[on].append(r.frames / r.seconds_total)
            off, on = float(np.median(fps[False])), float(np.median(fps[True]))
            print(f"evaluate_yuv, {fmt.name}, rescale_metrics=True, metrics only, {T} frames {H}x{W}, chunk {chunk}, end to end frames/s: "
                  f"{name} off per pass {' '.join('%.2f' % f for f in fps[False])}; median {off:.2f}; {name} on per pass "
                  f"{' '.join('%.2f' % f for f in fps[True])}; median {on:.2f} ({on / off:.4f} of off); mean {getattr(r, 'mean_' + name):.5f}",
                  flush=True)


if __name__ == "__main__":
    if "--rescale-metrics" in sys.argv:
        rescale_metrics()
    elif "--lpips" in sys.argv:
        lpips()
    elif "--tof" in sys.argv:
        tof()
    elif "--brisque" in sys.argv:
        brisque()
    elif "--niqe" in sys.argv:
        niqe()
    elif "--msssim" in sys.argv:
        msssim()
    elif "--ssim" in sys.argv:
        ssim_ab()
    elif "--yuv" in sys.argv:
        pix_fmt() if "--pix-fmt" in sys.argv else yuv()
    else:
        sequence()
