"""Developer benchmark (GPU box): the Gumbel hard-mask + 9-tap channel convolution kernel (cdfo_rdab_prep_rng, arch.py:2168-2219)
stand-alone at one neighbour of the bench shape (8 x 272 x 480); prints the time per launch and a fingerprint of its three outputs
(A/B builds through CDFO_LIB_PATH must agree except where a pixel's softmax sits within rounding of the 0.5 threshold).  Beside it,
on the same tensors: RDAB.input_conv (64 -> 128, streaming kernel) followed by that launch against the one launch that does both
(cdfo_rdab_prep_fused, fp32 and fp16 V outputs), for one neighbour and for a group of three (one 24-image conv + 3 launches
against 3 launches)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cdfo_amd import kernels as K


def _time(fn, n=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    B, H, W = 8, 272, 480
    g = torch.Generator(device="cuda").manual_seed(5)
    xq = torch.randn(B, H, W, 128, device="cuda", generator=g)
    vmax = torch.rand(B, 64, device="cuda", generator=g) * 2
    wW = torch.randn(1, 1, 1, 9, device="cuda", generator=g) * 0.3
    bW = torch.randn(1, device="cuda", generator=g) * 0.1
    noise = torch.empty(B, 64, H, W, device="cuda")
    outs = K.rdab_prep_rng(xq, vmax, 12345, 2, wW, bW, noise_out=noise)
    ref = K.rdab_prep(xq, vmax, noise, wW, bW)                      # the injected-noise entry on the captured noise: same kernel body
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(outs, ref))
    masked = (outs[2] == 0).float().mean().item()                   # share of (pixel, channel) with mask = 1 (window query zeroed)
    ms = _time(lambda: K.rdab_prep_rng(xq, vmax, 12345, 2, wW, bW, outs=outs))
    fp = [float(t.double().sum().item()) for t in outs]
    print(f"rdab_prep_rng {B}x{H}x{W}: {ms:.4f} ms per launch; rng == injected: {same}; masked share {masked:.5f}; "
          f"fingerprints {fp[0]:.6f} {fp[1]:.6f} {fp[2]:.6f}")

    # ---- input_conv + rdab_prep_rng against the fused launch, G neighbours of B images
    pc = K.pack_conv(torch.randn(128, 64, 1, 1, device="cuda", generator=g) / 8, torch.randn(128, device="cuda", generator=g) * 0.1)
    for G in (1, 3):
        x = torch.randn(G * B, H, W, 64, device="cuda", generator=g)
        vm = vmax.repeat(G, 1)
        xq_g = torch.empty(G * B, H, W, 128, device="cuda")
        old = tuple(torch.empty(G * B, H, W, 64, device="cuda") for _ in range(3))
        sls = [slice(i * B, (i + 1) * B) for i in range(G)]

        def two_kernels():
            K.conv(x, pc, prec=K.PREC_FP16X2, out=xq_g)
            for i, sl in enumerate(sls):
                K.rdab_prep_rng(xq_g[sl], vm[sl], 12345, i, wW, bW, outs=tuple(t[sl] for t in old))

        t_old = _time(two_kernels)
        line = f"input_conv + rdab_prep_rng {G * B}x{H}x{W}: {t_old:.4f} ms;  fused"
        for v_f16 in (False, True):
            vdt = torch.float16 if v_f16 else torch.float32
            new = tuple(torch.empty(G * B, H, W, 64, device="cuda", dtype=dt) for dt in (torch.float32, vdt, torch.float32, vdt))

            def fused():
                for i, sl in enumerate(sls):
                    K.rdab_prep_fused(x[sl], pc, vm[sl], ("rng", 12345, i, None), wW, bW, v_f16=v_f16, outs=tuple(t[sl] for t in new))

            t_new = _time(fused)
            ok = (torch.equal(new[0], old[0]) and torch.equal(new[2], old[2]) and torch.equal(new[1], old[1].to(vdt))
                  and torch.equal(new[3], xq_g[..., 64:].to(vdt)))
            line += f" ({'fp16' if v_f16 else 'fp32'} V) {t_new:.4f} ms, equal: {ok};"
        print(line)


if __name__ == "__main__":
    main()
