"""Developer benchmark (GPU box only): `cdfo_amd.loss.ssim_loss` and `msssim_loss` alone, beside the same expressions written with
torch.nn.functional.conv2d and autograd on the device (in fp64, as the definition is, and once more in fp32 to show what fp64 costs):

    python tools/bench_ssim_loss.py [N H W] [--passes 5]

Each pass times, by events, per loss: the project's forward (sr needs no gradient: sums, pools and the combine), its forward +
backward (the gradient passes run in the forward, the backward is one scaling), then the conv2d form's forward and forward +
backward -- so the forms alternate in one process -- and then each entry point on its own through the C ABI, at level 0 (the pool:
level 0 -> 1).  The figures are the medians over the passes behind one warm-up pass."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _window(device):
    k = torch.exp(-((torch.arange(11, dtype=torch.float64, device=device) - 5.0) ** 2) / (2 * 1.5 ** 2))
    return k / k.sum()                                                       # fp64; _means casts it to the planes' type


def _means(x, y, peak):
    """(M_cs, M_ssim) [N] of fp64 [N,1,h,w]: five planes through two separable conv2d calls."""
    g = _window(x.device).to(x.dtype)
    C1, C2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
    planes = torch.cat((x, y, x * x, y * y, x * y), dim=1)
    planes = F.conv2d(F.conv2d(planes, g.view(1, 1, 11, 1).expand(5, 1, 11, 1), groups=5), g.view(1, 1, 1, 11).expand(5, 1, 1, 11), groups=5)
    m1, m2, e11, e22, e12 = planes.unbind(dim=1)
    cs = (2 * (e12 - m1 * m2) + C2) / ((e11 - m1 * m1) + (e22 - m2 * m2) + C2)
    lum = (2 * m1 * m2 + C1) / (m1 * m1 + m2 * m2 + C1)
    return cs.mean(dim=(1, 2)), (lum * cs).mean(dim=(1, 2))


def torch_form(sr, hr, peak, levels, dtype=torch.float64):
    x, y = sr.to(dtype), hr.to(dtype)
    if levels == 1:
        return (1.0 - _means(x, y, peak)[1]).float()
    prod = 1.0
    for j in range(5):
        if j:
            x, y = (F.avg_pool2d(t, 2).float().to(dtype) for t in (x, y))    # rounds as the definition does; autograd goes through the cast
        m = _means(x, y, peak)[1 if j == 4 else 0]
        prod = prod * m.clamp(min=0) ** WEIGHTS[j]
    return (1.0 - prod).float()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    argv = list(sys.argv[1:])
    passes = 5
    if "--passes" in argv:
        at = argv.index("--passes")
        passes = int(argv[at + 1])
        del argv[at:at + 2]
    N, H, W = (int(a) for a in argv[:3]) if len(argv) >= 3 else (20, 256, 256)
    from cdfo_amd import _lib, kernels as K
    from cdfo_amd.loss import msssim_loss, ssim_loss
    gen = torch.Generator(device="cuda").manual_seed(1)
    hr = torch.rand(N, 1, H, W, device="cuda", generator=gen)
    sr0 = (hr + 0.1 * torch.randn(N, 1, H, W, device="cuda", generator=gen)).clamp(0, 1)
    sr = sr0.clone().requires_grad_(True)

    def both(fn):
        sr.grad = None
        fn(sr, hr).sum().backward()

    forms, absent = {}, []
    for name, fn, levels in (("ssim_loss", ssim_loss, 1), ("msssim_loss", msssim_loss, 5)):
        if min(H, W) < (176 if levels == 5 else 11):
            continue
        forms[f"{name}: hip forward"] = lambda fn=fn: fn(sr0, hr)
        forms[f"{name}: hip forward + backward"] = lambda fn=fn: both(fn)
        for dtype, tag in ((torch.float64, "fp64"), (torch.float32, "fp32, NOT the definition")):
            ref = lambda a, b, levels=levels, dtype=dtype: torch_form(a, b, 1.0, levels, dtype)       # noqa: E731
            try:
                both(ref)
            except RuntimeError as e:
                absent.append(f"{name}: conv2d in {tag} on the device: not available in this build ({str(e).splitlines()[0]})")
                continue
            forms[f"{name}: conv2d ({tag}) forward"] = lambda ref=ref: ref(sr0, hr)
            forms[f"{name}: conv2d ({tag}) + autograd forward + backward"] = lambda ref=ref: both(ref)
    # the entry points on their own, at level 0 of the one-scale loss
    lib, vp, st = _lib.lib(), _lib._vp, K._stream
    T = lib.cdfo_ssim_loss_tiles(H, W, 1)
    f64 = dict(dtype=torch.float64, device="cuda")
    partial, means, coef = torch.empty((N, T, 2), **f64), torch.empty((N, 1, 2), **f64), torch.empty((N, 1, 2), **f64)
    loss, g = torch.empty(N, device="cuda"), torch.empty_like(sr0)
    pqr = torch.empty((N, 3, H - 10, W - 10), **f64)
    xn, yn = torch.empty((N, H // 2, W // 2), device="cuda"), torch.empty((N, H // 2, W // 2), device="cuda")
    parts = {
        "cdfo_ssim_loss_level": lambda: lib.cdfo_ssim_loss_level(vp(sr0), vp(hr), N, H, W, 1, 0, 1.0, vp(partial), partial.numel(), st()),
        "cdfo_ssim_loss_pool": lambda: lib.cdfo_ssim_loss_pool(vp(sr0), vp(hr), N, H, W, vp(xn), vp(yn), st()),
        "cdfo_ssim_loss_combine": lambda: lib.cdfo_ssim_loss_combine(vp(partial), partial.numel(), N, H, W, 1, vp(means), vp(coef), vp(loss), st()),
        "cdfo_ssim_loss_pqr": lambda: lib.cdfo_ssim_loss_pqr(vp(sr0), vp(hr), N, H, W, 1, 0, 1.0, vp(coef), vp(pqr), pqr.numel(), st()),
        "cdfo_ssim_loss_adjoint": lambda: lib.cdfo_ssim_loss_adjoint(vp(pqr), vp(sr0), vp(hr), N, H, W, 1, 0, None, None, vp(g), st()),
    }
    px, po = N * H * W, N * (H - 10) * (W - 10)
    moved = {"cdfo_ssim_loss_level": 8 * px, "cdfo_ssim_loss_pool": 10 * px, "cdfo_ssim_loss_pqr": 8 * px + 24 * po,
             "cdfo_ssim_loss_adjoint": 24 * po + 12 * px}                    # compulsory traffic: inputs once, outputs once
    times = {k: [] for k in list(forms) + list(parts)}
    for it in range(passes + 1):
        for k, fn in list(forms.items()) + list(parts.items()):
            t = timed(fn)
            if it:
                times[k].append(t)
    print(f"ssim_loss / msssim_loss {N}x1x{H}x{W}, medians of {passes} (passes min - max), forms alternating in one process")
    for k, v in times.items():
        tail = ""
        if k in moved:
            tail = f"; one launch, {moved[k] / 2**20:.1f} MiB moved, {moved[k] / statistics.median(v) / 1e6:.0f} GB/s"
        print(f"  {k}: {statistics.median(v) * 1e3:.1f} us ({min(v) * 1e3:.1f} - {max(v) * 1e3:.1f}){tail}")
    for line in absent:
        print("  " + line)
    for name, fn, levels in (("ssim_loss", ssim_loss, 1), ("msssim_loss", msssim_loss, 5)):
        if f"{name}: conv2d (fp64) forward" in forms:
            a, b = fn(sr0, hr), torch_form(sr0, hr, 1.0, levels)
            print(f"  {name}: the two forms' losses differ by at most {float((a - b).abs().max()):.2g}")


if __name__ == "__main__":
    main()
