"""Developer benchmark (GPU box): LLongRangAttention's mask statistics stand-alone at a neighbour group of the bench shape (3 slots x
8 windows of 272 x 480): the three stem_conv2 launches + the exact-mode conv_du_re.2 over the space-to-depth du0 + chan_sum_partial
(stem_conv2's other output, fea_com, is timed apart as the three stem_conv launches that remain) against the one cdfo_rdab_stats
launch.  Prints the times per group and the largest difference of the channel means, relative to max |mean|."""
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
    B, G, H, W = 8, 3, 272, 480
    P = H * W
    g = torch.Generator(device="cuda").manual_seed(5)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    rms = r(B, 1, 7, H, W) * 0.2
    w_rms, b_rms, w_du0, b_du0, w2, b2 = r(64, 1, 3, 3) / 3, r(64) * 0.1, r(64, 64, 1, 1) / 8, r(64) * 0.1, r(64, 64, 3, 3) / 24, r(64) * 0.1
    w0, b0 = K.compose_stem_1x1(w_rms, b_rms, w_du0, b_du0)
    pc, img = K.pack_conv_s2p2_s2d(w2, b2), K.pack_rdab_stats(w2)
    fea = r(G * B, H, W, 64)
    fea_com = torch.empty_like(fea)
    du0 = torch.zeros(G * B, H // 2 + 1, W // 2 + 1, 256, device="cuda")
    sls = [slice(i * B, (i + 1) * B) for i in range(G)]

    def stems2():
        for i, sl in enumerate(sls):
            K.stem_conv2(rms[:, 0, i], 7 * P, B, H, W, w_rms, b_rms, fea[sl], fea_com[sl], w0, b0, K.ACT_RELU, du0[sl], s2dB=True)

    def stems1():
        for i, sl in enumerate(sls):
            K.stem_conv(rms[:, 0, i], 7 * P, B, H, W, w_rms, b_rms, add=fea[sl], out2=fea_com[sl], write_out=False)

    def old_stats():
        return K.chan_sum_partial(K.conv(du0, pc, pad=1, act=K.ACT_RELU, prec=K.PREC_BF16X3))

    def new_stats():
        return K.rdab_stats(rms[:, 0, 0], B, 7 * P, P, G * B, H, W, w0, b0, img, b2)

    stems2()
    po, pn = old_stats()[0], new_stats()[0]
    mo, mn = po.double().sum(1), pn.double().sum(1)
    diff = ((mo - mn).abs().max() / mo.abs().max()).item()
    t = [_time(f) for f in (stems2, stems1, old_stats, new_stats)]
    print(f"mask statistics {G}x{B}x{H}x{W}: stem_conv2 x3 {t[0]:.4f} ms + conv + chan_sum {t[2]:.4f} ms = {t[0] + t[2]:.4f} ms;  "
          f"stem_conv x3 {t[1]:.4f} ms + rdab_stats {t[3]:.4f} ms = {t[1] + t[3]:.4f} ms;  means differ by {diff:.2e} rel")


if __name__ == "__main__":
    main()
