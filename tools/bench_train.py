"""Developer benchmark (GPU box only): one training step of CVSR_V8 at the reference script's batch (train_LD_37.py: 20 crops of
64x64, Charbonnier loss) -- forward and backward through the HIP autograd path, timed separately.

    python tools/bench_train.py [B H W] [--lpips random | --ffl | --ssim [1|5]]

--lpips random: passes with and without the perceptual term alternate in one process; the term is 0.1 * cdfo_amd.loss.lpips_loss with a
seeded random trunk of the published widths (metrics.lpips_random_params), its forward counted with the forward.
--ffl: the same alternation with and without the frequency term, 1.0 * cdfo_amd.loss.focal_frequency_loss (its inverse passes run in
the forward, as Charbonnier's derivative does); B H W then need 4 H and 4 W powers of two up to 512.
--ssim [1|5]: the same alternation with and without the structural term, 1.0 * cdfo_amd.loss.ssim_loss (1, the default) or msssim_loss
(5; 4 H and 4 W must then be at least 176); its gradient passes run in the forward, too."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from arch.SIDECVSR_our import CVSR_V8
from _inputs import random_inputs


def main():
    argv = list(sys.argv[1:])
    lpips = None
    if "--lpips" in argv:
        at = argv.index("--lpips")
        if argv[at + 1:at + 2] != ["random"]:
            sys.exit("bench_train: --lpips takes `random`")
        del argv[at:at + 2]
        from cdfo_amd.loss import lpips_loss
        from cdfo_amd.metrics import lpips_random_params
        lpips = lpips_random_params()
    ffl = "--ffl" in argv
    if ffl:
        argv.remove("--ffl")
        if lpips is not None:
            sys.exit("bench_train: --lpips or --ffl, one at a time")
        from cdfo_amd.loss import focal_frequency_loss
    ssim = 0
    if "--ssim" in argv:
        at = argv.index("--ssim")
        given = argv[at + 1:at + 2] in (["1"], ["5"]) and len(argv) - 2 in (0, 3)      # else the next word is B of `B H W`
        ssim = int(argv[at + 1]) if given else 1
        del argv[at:at + 1 + given]
        if lpips is not None or ffl:
            sys.exit("bench_train: --lpips, --ffl or --ssim, one at a time")
        from cdfo_amd.loss import msssim_loss, ssim_loss
        structural = ssim_loss if ssim == 1 else msssim_loss
    B, H, W = (int(a) for a in argv[:3]) if len(argv) >= 3 else (20, 64, 64)
    m = CVSR_V8().cuda().train()
    inp = random_inputs(B, H, W, 7)
    d = {k: v.cuda() for k, v in inp.items() if k != "gumbel_u"}
    hr = torch.rand(B, 1, 4 * H, 4 * W, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    extra = lpips is not None or ffl or bool(ssim)
    for it in range(12 if extra else 4):
        with_lpips = lpips is not None and it % 2 == 1
        with_ffl = ffl and it % 2 == 1
        with_ssim = bool(ssim) and it % 2 == 1
        m.zero_grad(set_to_none=True)
        ev[0].record()
        out, _ = m(d["x"], d["mvs0"], d["mvs1"], d["pms"], d["rms"], d["ufs"])
        loss = torch.sum(torch.sqrt((out - hr) ** 2 + 1e-4))
        if with_lpips:
            loss = loss + 0.1 * lpips_loss(out, hr, lpips).sum()
        if with_ffl:
            loss = loss + focal_frequency_loss(out, hr).sum()
        if with_ssim:
            loss = loss + structural(out, hr).sum()
        ev[1].record()
        loss.backward()
        ev[2].record()
        torch.cuda.synchronize()
        if it > (1 if extra else 0):
            print(f"training step {B}x{H}x{W}{' + lpips' if with_lpips else ' + ffl' if with_ffl else ' + ssim' if with_ssim and ssim == 1 else ' + msssim' if with_ssim else ''}: forward {ev[0].elapsed_time(ev[1]):.1f} ms, backward {ev[1].elapsed_time(ev[2]):.1f} ms", flush=True)


if __name__ == "__main__":
    main()
