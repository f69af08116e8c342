"""Developer benchmark (GPU box): the in-place feature stack stand-alone at the bench shape (8 clips x 7 frames of 272 x 480, a
neighbour group of 3 frames).
  the copies that go (model.stack_inplace): K.swap_outer of the 56-frame stack and the centre features repeated three times over,
      against nothing;
  each of the seven readers on a mapped operand taken from the clip-major stack   against   the same launch on the dense copy of
      those images: a reader that got slower on strided images would show here."""
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
    B, N, G, H, W = 8, 7, 3, 272, 480
    P, M = H * W, 24
    g = torch.Generator(device="cuda").manual_seed(5)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    L1 = r(B * N, H, W, 64)                                     # clip-major, as the extractor writes it
    first = lambda i: L1.view(B, N, H, W, 64)[0, i]
    grp = K.image_map(first(0), M, B, N * P * 64, P * 64)       # frames 0-2 of every clip
    ctr = K.image_map(first(3), M, B, N * P * 64, 0)            # the centre once per neighbour
    ctr1 = K.image_map(first(3), B, B, N * P * 64, 0)           # the centre of every clip
    Lf = K.swap_outer(L1, B, N).view(N, B, H, W, 64)
    fea, xcG, xc1 = Lf[0:3].reshape(M, H, W, 64), Lf[3].repeat(G, 1, 1, 1), Lf[3]
    t = [_time(f) for f in (lambda: K.swap_outer(L1, B, N), lambda: Lf[3].repeat(G, 1, 1, 1))]
    print(f"the copies {B}x{N}x{H}x{W}: swap_outer {t[0]:.4f} + repeat x{G} {t[1]:.4f} = {t[0] + t[1]:.4f} ms per forward; in place: 0")

    rms = r(B, 1, 7, H, W) * 0.2
    ws, bs = r(64, 1, 3, 3) / 3, r(64) * 0.1
    wi, bi = r(128, 64, 1, 1) / 8, r(128) * 0.1
    wf, bf = r(64, 128, 1, 1) / 11, r(64) * 0.1
    pci, pcf = K.pack_conv(wi, bi), K.pack_conv(wf, bf)
    t_in = K.pack_plane_chunk(*K.compose_stem_1x1(ws, bs, wi, torch.zeros_like(bi)))
    t_res = K.pack_plane_chunk(ws, bs)
    addr = (rms[:, 0, 0], B, 7 * P, P)
    vmax = 3.0 * torch.rand(M, 64, device="cuda", generator=g)
    wW, bW = r(1, 1, 1, 9) * 0.4, r(1)
    outs = tuple(torch.empty(M, H, W, 64, device="cuda", dtype=dt) for dt in (torch.float32, torch.float32, torch.float32, torch.float16))
    out = torch.empty(M, H, W, 64, device="cuda")
    sls = [slice(i * B, (i + 1) * B) for i in range(G)]
    rows = []

    def prep(x):
        for i, sl in enumerate(sls):
            xs = x.sub(i * B, B) if isinstance(x, K.ImageMap) else x[sl]
            K.rdab_prep_fused(xs, pci, vmax[sl], ("rng", 1234, i, None), wW, bW, v_f16=(False, True), outs=tuple(o[sl] for o in outs),
                              plane=(rms[:, 0, i], B, 7 * P, 0, t_in))
    rows.append(("rdab_prep_fused x3 (x)", lambda: prep(fea), lambda: prep(grp)))

    cat = r(M, H, W, 128)
    rows.append(("RDAB.fuse (res1)", lambda: K.conv(cat, pcf, res1=fea, out=out, prec=K.PREC_FP16X2, plane=(*addr, t_res)),
                 lambda: K.conv(cat, pcf, res1=grp, out=out, prec=K.PREC_FP16X2, plane=(*addr, t_res))))

    x_n = r(M, H, W, 64)
    pc3 = K.pack_conv(r(64, 128, 3, 3) / 34, r(64) * 0.1)
    rows.append(("conv_expand_fea_r (source 0)", lambda: K.conv([fea, x_n], pc3, pad=1, out=out, prec=K.PREC_FP16X2),
                 lambda: K.conv([grp, x_n], pc3, pad=1, out=out, prec=K.PREC_FP16X2)))

    x0 = r(M, H, W, 64)
    t_stats = K.pack_plane_chunk(*K.compose_stem_1x1(ws, bs, wf[:, 64:], torch.zeros_like(bs)))
    rows.append(("align_stats (q)", lambda: K.align_stats(x0, None, xcG, pcf, K.ACT_RELU, 16, plane=(*addr, t_stats, t_res)),
                 lambda: K.align_stats(x0, None, ctr, pcf, K.ACT_RELU, 16, plane=(*addr, t_stats, t_res))))

    wb = r(M, 64, 128) / 11
    pk = lambda w: torch.cat([K.pack_conv(w[m].reshape(64, -1, 1, 1).contiguous(), None).w for m in range(M)])
    pc128 = K.PackedConv(pk(wb), bf, 64, 128, 1, 64, w_bstride=128 * 64)
    tables = torch.stack([K.pack_plane_chunk(*K.compose_stem_1x1(ws, bs, wb[m, :, 64:128].reshape(64, 64, 1, 1), torch.zeros_like(bs)))
                          for m in range(M)]).contiguous()
    kw = dict(act=K.ACT_RELU, out=out, prec=K.PREC_FP16X2, chan_sum_out=True, plane=(*addr, tables, 1024))
    rows.append(("folded 128->64 with sums (xc)", lambda: K.conv([x0, xcG], pc128, **kw), lambda: K.conv([x0, ctr], pc128, **kw)))

    pcr = K.pack_conv(r(64, 64, 3, 3) / 24, r(64) * 0.1)
    x16 = K.to_cp16(x0)
    rows.append(("conv3x3_ws_res (res2)", lambda: K.conv3x3_ws_res(x16, pcr, res1=x_n, res2=xcG, out=out),
                 lambda: K.conv3x3_ws_res(x16, pcr, res1=x_n, res2=ctr, out=out)))

    al = [r(B, H, W, 64) for _ in range(6)]
    pct = K.pack_conv(r(64, 448, 1, 1) / 21, r(64) * 0.1)
    o1 = torch.empty(B, H, W, 64, device="cuda")
    rows.append(("tsa_fusion (centre)", lambda: K.conv([*al[:3], xc1, *al[3:]], pct, act=K.ACT_LRELU, out=o1, prec=K.PREC_FP16X2),
                 lambda: K.conv([*al[:3], ctr1, *al[3:]], pct, act=K.ACT_LRELU, out=o1, prec=K.PREC_FP16X2)))

    for name, dense, mapped in rows:
        td, tm = _time(dense), _time(mapped)
        print(f"{name:34s} dense {td:.4f} ms   mapped {tm:.4f} ms   ({tm - td:+.4f})")


if __name__ == "__main__":
    main()
