"""LLongRangAttention's mask statistics straight from the residual maps (`kernels.rdab_stats`: neither du0 = relu(conv_du_re.0(
conv_expand_rms(rms))) nor relu(conv_du_re.2(du0)) is written) against the three launches it replaces: stem_conv2 (du0 in
space-to-depth form) -> the exact-mode convolution -> chan_sum_partial.

Bounds.  Both paths form du0 with the same nine fp32 FMAs and multiply it as split-bf16 hi | lo in three MFMA passes with fp32
accumulation; the order of the 576 products and the grouping of the pixel sums differ.  So each is measured against a float64
restatement NEXT TO the other, and the new kernel may show at most 4 x the replaced path's error (the rule of
tests/test_gpu_align_stats.py).  Compared is what the consumer uses: the channel means relative to max |mean|, and vmax =
relu(conv_du_re2.0(mean)) after vec_mlp, absolute.  Forward with the switch off / on: the returned features must be identical (the
statistics do not reach them), the image within a tenth of the forward's parity bound.

Measured on MI355X (means rel / vmax abs; replaced path -> rdab_stats), float64 restatement as the reference:
    2x8x8                1.09e-06 / 2.00e-07  ->  1.34e-06 / 3.81e-07
    2x10x14              1.42e-06 / 2.62e-07  ->  1.62e-06 / 3.79e-07
    1x24x40              1.44e-06 / 3.03e-07  ->  1.67e-06 / 5.12e-07
    1x64x64              1.38e-06 / 2.93e-07  ->  1.52e-06 / 5.27e-07
    3x272x480            1.48e-06 / 4.14e-07  ->  1.75e-06 / 6.15e-07
    3x2x8x8 (strided)    2.68e-06 / 5.76e-07  ->  2.21e-06 / 7.06e-07
    3x2x8x16 (strided)   1.83e-06 / 5.72e-07  ->  1.90e-06 / 7.06e-07
    3x2x38x54 (strided)  1.75e-06 / 7.69e-07  ->  1.88e-06 / 8.14e-07
(the stem block forms du0 by a split-bf16 product where the replaced path used fp32 FMAs: its 2^-17 joins the convolution's).
Forward with the switch off / on, both cases: out and L1_fea bitwise equal (vmax feeds only the mask's 0.5 threshold).
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _weights(seed):
    """(w_rms [64,1,3,3], b_rms, w_du0 [64,64,1,1], b_du0, w2 [64,64,3,3], b2, w3 [64,64,1,1], b3) seeded on the CPU"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return [t.cuda() for t in (r(64, 1, 3, 3) / 3, r(64) * 0.1, r(64, 64, 1, 1) / 8, r(64) * 0.1, r(64, 64, 3, 3) / 24, r(64) * 0.1,
                               r(64, 64, 1, 1) / 8, r(64) * 0.1)]


def _maps(B, H, W, seed):
    """a [B,1,7,H,W] stack of residual maps (signed, a third of the samples zero: flat regions)"""
    g = torch.Generator().manual_seed(seed)
    m = torch.randn(B, 1, 7, H, W, generator=g) * 0.2
    return (m * (torch.rand(B, 1, 7, H, W, generator=g) > 0.33)).cuda()


def _restatement(planes, w0, b0, w2, b2, w3, b3):
    """float64: planes [M,H,W] -> (channel means [M,64] of relu(conv_du_re.2(du0)), vmax [M,64]); shifted products, no library conv"""
    M, H, W = planes.shape
    Ho, Wo = H // 2 + 1, W // 2 + 1
    x = torch.zeros(M, H + 2, W + 2, dtype=torch.float64, device=planes.device)
    x[:, 1:-1, 1:-1] = planes.double()
    du0 = b0.double().view(1, 64, 1, 1).repeat(M, 1, H, W)
    for u in range(9):
        du0 += w0.double().view(64, 9)[:, u].view(1, 64, 1, 1) * x[:, None, u // 3:u // 3 + H, u % 3:u % 3 + W]
    pad = torch.zeros(M, 64, H + 4, W + 4, dtype=torch.float64, device=planes.device)      # the padding is du0's: zeros, not relu(bias)
    pad[:, :, 2:-2, 2:-2] = torch.relu(du0)
    t = b2.double().view(1, 64, 1, 1).repeat(M, 1, Ho, Wo)
    for ky in range(3):
        for kx in range(3):
            t += torch.einsum("oc,mchw->mohw", w2.double()[:, :, ky, kx], pad[:, :, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2])
    mean = torch.relu(t).mean((2, 3))
    return mean, torch.relu(mean @ w3.double().view(64, 64).t() + b3.double())


def _fold_mean(part, count):
    s = torch.zeros_like(part[:, 0])
    for ch in range(part.shape[1]):
        s = s + part[:, ch]
    return s.double() / count


def _old_path(views, bstride, H, W, wts):
    """the replaced launches on the planes views[k] [Bk,H,W] (image b at b * bstride): partials [M,n,64], n"""
    from cdfo_amd import kernels as K
    w_rms, b_rms, w_du0, b_du0, w2, b2, _, _ = wts
    w0, b0 = K.compose_stem_1x1(w_rms, b_rms, w_du0, b_du0)
    M = sum(v.shape[0] for v in views)
    fea = torch.zeros(M, H, W, 64, device="cuda")
    du0 = torch.zeros(M, H // 2 + 1, W // 2 + 1, 256, device="cuda")
    m0 = 0
    for v in views:
        sl = slice(m0, m0 + v.shape[0])
        K.stem_conv2(v, bstride, v.shape[0], H, W, w_rms, b_rms, fea[sl], torch.empty_like(fea[sl]), w0, b0, K.ACT_RELU, du0[sl], s2dB=True)
        m0 = sl.stop
    t = K.conv(du0, K.pack_conv_s2p2_s2d(w2, b2), pad=1, act=K.ACT_RELU, prec=K.PREC_BF16X3)
    return K.chan_sum_partial(t)


def _new_path(base, Bi, s_b, s_g, M, H, W, wts):
    from cdfo_amd import kernels as K
    w_rms, b_rms, w_du0, b_du0, w2, b2, _, _ = wts
    w0, b0 = K.compose_stem_1x1(w_rms, b_rms, w_du0, b_du0)
    return K.rdab_stats(base, Bi, s_b, s_g, M, H, W, w0, b0, K.pack_rdab_stats(w2), b2)


def _vmax(part, n, count, wts):
    from cdfo_amd import kernels as K
    return K.vec_mlp(part, n, count, wts[6], wts[7], 64, K.ACT_RELU).double()


def _compare(tag, maps, slots, H, W, wts):
    """slots: the consecutive slots i0 .. i0+G-1 of maps [B,1,7,H,W]; images are slot major, as a neighbour group's"""
    B, P = maps.shape[0], H * W
    views = [maps[:, 0, i] for i in slots]
    planes = torch.cat(views, 0)
    M = planes.shape[0]
    w_rms, b_rms, w_du0, b_du0, w2, b2, w3, b3 = wts
    from cdfo_amd import kernels as K
    w0, b0 = K.compose_stem_1x1(w_rms, b_rms, w_du0, b_du0)
    ref_mean, ref_vmax = _restatement(planes, w0, b0, w2, b2, w3, b3)
    count = (H // 2 + 1) * (W // 2 + 1)
    po, no = _old_path(views, 7 * P, H, W, wts)
    pn, nn, cn = _new_path(views[0], B, 7 * P, P, M, H, W, wts)
    assert cn == count and pn.shape == (M, nn, 64) and nn == no
    scale = ref_mean.abs().max()
    old = (((_fold_mean(po, count) - ref_mean).abs().max() / scale).item(), (_vmax(po, no, count, wts) - ref_vmax).abs().max().item())
    new = (((_fold_mean(pn, count) - ref_mean).abs().max() / scale).item(), (_vmax(pn, nn, count, wts) - ref_vmax).abs().max().item())
    torch.cuda.synchronize()
    print(f"rdab_stats {tag}: means rel {old[0]:.2e} -> {new[0]:.2e}, vmax abs {old[1]:.2e} -> {new[1]:.2e}, slots {nn}, "
          f"max |mean| {scale.item():.3f}, vmax > 0: {(ref_vmax > 0).sum().item()} of {ref_vmax.numel()}")
    assert new[0] <= 4 * old[0], f"rdab_stats means {(old, new)}"
    assert new[1] <= 4 * old[1], f"rdab_stats vmax {(old, new)}"


@pytest.mark.parametrize("B,H,W", [(2, 8, 8), (2, 10, 14), (1, 24, 40), (1, 64, 64), (3, 272, 480)])
def test_rdab_stats_against_float64(B, H, W):
    _compare(f"{B}x{H}x{W}", _maps(B, H, W, 300 + H), [2], H, W, _weights(17))


@pytest.mark.parametrize("H,W", [(8, 8), (8, 16), (38, 54)])
def test_rdab_stats_group_through_plane_strides(H, W):
    """6 images as 3 slots x 2 windows of a [2,1,7,H,W] tensor in ONE launch (image m at (m % 2) 7 P + (m // 2) P), against the
    replaced path's three stem launches; the last slots of the tensor, so that a stride error reads beyond it"""
    _compare(f"3x2x{H}x{W} strided", _maps(2, H, W, 77 + W), [4, 5, 6], H, W, _weights(18))


def test_odd_sizes_stay_on_the_old_path():
    from cdfo_amd import kernels as K
    assert K.rdab_stats_ok(24, 40) and not K.rdab_stats_ok(9, 14) and not K.rdab_stats_ok(10, 13)
    wts = _weights(3)
    with pytest.raises(ValueError):
        _new_path(_maps(1, 9, 14, 1)[:, 0, 0], 1, 7 * 9 * 14, 0, 1, 9, 14, wts)


def _dump(path):
    """the partials of one seeded call (a group through the plane strides, several chunks per image) -> path"""
    maps = _maps(2, 72, 120, 4242)
    part, _, _ = _new_path(maps[:, 0, 1], 2, 7 * 72 * 120, 72 * 120, 6, 72, 120, _weights(19))
    torch.cuda.synchronize()
    arr = part.cpu().numpy()
    if path:
        np.save(path, arr)
    return arr


def test_partials_are_bitwise_reproducible(tmp_path):
    from conftest import clean_process_run
    first, second = _dump(None), _dump(None)
    assert first.tobytes() == second.tobytes()
    path = str(tmp_path / "partials.npy")
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_gpu_rdab_stats as t; t._dump({path!r})"
    rc, so, se = clean_process_run([sys.executable, "-c", code], cwd=ROOT, timeout=120)
    assert rc == 0, se[-2000:]
    assert first.tobytes() == np.load(path).tobytes()


@pytest.mark.parametrize("B,H,W,seed", [(1, 24, 40, None), (1, 64, 64, 910)])
def test_forward_with_and_without_the_prior_stems(B, H, W, seed):
    """model.prior_stems (CDFO_PRIOR_STEMS) off and on, injected noise: L1_fea identical, out within a tenth of the forward's parity
    bound (1e-3: regrouped fp32 sums in 64 statistics per image); the first case is the 24x40 golden and is also held to the golden."""
    from arch.SIDECVSR_our import CVSR_V8
    from oracle.cvsr_v8_ref import make_inputs, make_state_dict
    gold = None
    if seed is None:
        gold = np.load(os.path.join(ROOT, "tests", "golden", "cvsr_v8_b1_24x40.npz"))
        wseed, seed, layout = int(gold["wseed"]), int(gold["iseed"]), str(gold["layout"])
    else:
        wseed, layout = 21, "b1n"
    m = CVSR_V8()
    m.load_state_dict(make_state_dict(wseed), strict=True)
    m = m.cuda().eval()
    inp = make_inputs(B, H, W, seed, layout)
    dev = {k: v.cuda() for k, v in inp.items() if k != "gumbel_u"}
    noise = [u.cuda() for u in inp["gumbel_u"]]
    res = {}
    with torch.no_grad():
        for on in (False, True):
            m.prior_stems = on
            out, l1 = m(dev["x"], dev["mvs0"], dev["mvs1"], dev["pms"], dev["rms"], dev["ufs"], gumbel_uniform=noise)
            res[on] = (out.clone(), l1.clone())
    torch.cuda.synchronize()
    d_out = (res[True][0] - res[False][0]).abs().max().item()
    print(f"prior_stems off/on {B}x{H}x{W}: out {d_out:.2e}")
    assert torch.equal(res[True][1], res[False][1])
    assert d_out <= 1e-4
    if gold is not None:
        assert (res[True][0].cpu() - torch.from_numpy(gold["out"])).abs().max().item() <= 1e-3
