"""Developer benchmark (GPU box): the plane chunk stand-alone at a neighbour group of the bench shape (3 slots x 8 windows of 272 x 480),
each changed launch next to what it replaces.
  rms half (model.inline_rms): 3 x stem_conv (fea_com = fea + conv_expand_rms(rms)) + 3 x rdab_prep_fused(fea_com) + RDAB.fuse with
      res1 = fea_com   against   3 x rdab_prep_fused(fea, plane) + RDAB.fuse with res1 = fea and the plane.
  K-block form: 3 x stem_conv (the 64-channel operand) + the per-image 192 -> 64 convolution with channel sums
      against   the 128 -> 64 convolution with the plane.
  ufs half (model.inline_ufs), the alignment's whole chain: 3 x stem_conv (ufs_prior) + align_stats + align_fold + the 192 -> 64
      convolution with channel sums   against   align_stats(plane) + align_fold_plane + the 128 -> 64 convolution with the plane."""
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
    P, M = H * W, 24
    g = torch.Generator(device="cuda").manual_seed(5)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    rms = r(B, 1, 7, H, W) * 0.2
    ws, bs = r(64, 1, 3, 3) / 3, r(64) * 0.1
    wi, bi = r(128, 64, 1, 1) / 8, r(128) * 0.1
    wf, bf = r(64, 128, 1, 1) / 11, r(64) * 0.1
    pci, pcf = K.pack_conv(wi, bi), K.pack_conv(wf, bf)
    t_in = K.pack_plane_chunk(*K.compose_stem_1x1(ws, bs, wi, torch.zeros_like(bi)))
    t_res = K.pack_plane_chunk(ws, bs)
    fea, cat = r(M, H, W, 64), r(M, H, W, 128)
    fea_com = torch.empty_like(fea)
    vmax = 3.0 * torch.rand(M, 64, device="cuda", generator=g)
    wW, bW = r(1, 1, 1, 9) * 0.4, r(1)
    outs = tuple(torch.empty(M, H, W, 64, device="cuda", dtype=dt) for dt in (torch.float32, torch.float32, torch.float32, torch.float16))
    out = torch.empty(M, H, W, 64, device="cuda")
    sls = [slice(i * B, (i + 1) * B) for i in range(G)]
    addr = (rms[:, 0, 0], B, 7 * P, P)

    def stems():
        for i, sl in enumerate(sls):
            K.stem_conv(rms[:, 0, i], 7 * P, B, H, W, ws, bs, add=fea[sl], out2=fea_com[sl], write_out=False)

    def prep(x, plane):
        for i, sl in enumerate(sls):
            pl = None if not plane else (rms[:, 0, i], B, 7 * P, 0, t_in)
            K.rdab_prep_fused(x[sl], pci, vmax[sl], ("rng", 1234, i, None), wW, bW, v_f16=(False, True), outs=tuple(o[sl] for o in outs), plane=pl)

    fuse_old = lambda: K.conv(cat, pcf, res1=fea_com, out=out, prec=K.PREC_FP16X2)
    fuse_new = lambda: K.conv(cat, pcf, res1=fea, out=out, prec=K.PREC_FP16X2, plane=(*addr, t_res))
    stems()
    t = [_time(f) for f in (stems, lambda: prep(fea_com, False), lambda: prep(fea, True), fuse_old, fuse_new)]
    print(f"rms half {G}x{B}x{H}x{W}: stem_conv x3 {t[0]:.4f} + rdab_prep_fused x3 {t[1]:.4f} + fuse {t[3]:.4f} = {t[0] + t[1] + t[3]:.4f} ms;  "
          f"with the plane: rdab_prep_fused x3 {t[2]:.4f} + fuse {t[4]:.4f} = {t[2] + t[4]:.4f} ms")

    # the K-block form with per-image weights and channel sums
    wb = r(M, 64, 192) / 13
    pk = lambda w: torch.cat([K.pack_conv(w[m].reshape(64, -1, 1, 1).contiguous(), None).w for m in range(M)])
    pc192 = K.PackedConv(pk(wb), bf, 64, 192, 1, 64, w_bstride=192 * 64)
    pc128 = K.PackedConv(pk(torch.cat([wb[:, :, :64], wb[:, :, 128:]], 2)), bf, 64, 128, 1, 64, w_bstride=128 * 64)
    tables = torch.stack([K.pack_plane_chunk(*K.compose_stem_1x1(ws, bs, wb[m, :, 64:128].reshape(64, 64, 1, 1), torch.zeros_like(bs)))
                          for m in range(M)]).contiguous()
    x0, x2, pred = r(M, H, W, 64), r(M, H, W, 64), torch.empty(M, H, W, 64, device="cuda")

    def stems_k():
        for i, sl in enumerate(sls):
            K.stem_conv(rms[:, 0, i], 7 * P, B, H, W, ws, bs, out=pred[sl])

    k_old = lambda: K.conv([x0, pred, x2], pc192, act=K.ACT_RELU, out=out, prec=K.PREC_FP16X2, chan_sum_out=True)
    k_new = lambda: K.conv([x0, x2], pc128, act=K.ACT_RELU, out=out, prec=K.PREC_FP16X2, chan_sum_out=True, plane=(*addr, tables, 1024))
    stems_k()
    t = [_time(f) for f in (stems_k, k_old, k_new)]
    print(f"K-block form {G}x{B}x{H}x{W}: stem_conv x3 {t[0]:.4f} + 192->64 with sums {t[1]:.4f} = {t[0] + t[1]:.4f} ms;  "
          f"128->64 with the plane and sums {t[2]:.4f} ms")

    # the alignment half: statistics, fold and the folded convolution on both paths
    q = r(M, H, W, 64)
    t_stats = K.pack_plane_chunk(*K.compose_stem_1x1(ws, bs, wf[:, 64:], torch.zeros_like(bs)))
    par = (r(4).abs() + 0.5, r(4, 64) * 0.2, r(4) * 0.1, r(64, 4) * 0.5, r(64) * 0.1, r(64, 64) / 8, wf.view(64, 128).contiguous())
    st_old = lambda: K.align_stats(x0, pred, q, pcf, K.ACT_RELU, 16)
    st_new = lambda: K.align_stats(x0, None, q, pcf, K.ACT_RELU, 16, plane=(*addr, t_stats, t_res))
    gp, s0, s1, n = st_old()
    fo_old = lambda: K.align_fold(gp, n, s0, s1, n, P, *par)
    fo_new = lambda: K.align_fold_plane(gp, n, s0, s1, n, P, *par, t_res)
    f192, (f128, ftab) = fo_old(), fo_new()
    c_old = lambda: K.conv([x0, pred, q], f192, act=K.ACT_RELU, out=out, prec=K.PREC_FP16X2, chan_sum_out=True)
    c_new = lambda: K.conv([x0, q], f128, act=K.ACT_RELU, out=out, prec=K.PREC_FP16X2, chan_sum_out=True, plane=(*addr, ftab, 1024))
    t = [_time(f) for f in (stems_k, st_old, fo_old, c_old, st_new, fo_new, c_new)]
    print(f"ufs half {G}x{B}x{H}x{W}: stem_conv x3 {t[0]:.4f} + align_stats {t[1]:.4f} + align_fold {t[2]:.4f} + 192->64 with sums {t[3]:.4f} = "
          f"{sum(t[:4]):.4f} ms;  with the plane: align_stats {t[4]:.4f} + align_fold_plane {t[5]:.4f} + 128->64 with sums {t[6]:.4f} = "
          f"{sum(t[4:]):.4f} ms")


if __name__ == "__main__":
    main()
