"""DualAttAlignment's statistics in one pass (`kernels.align_stats`: kf = relu(fusion_out.0([warped, pred])) is never written)
and the channel sums that the streaming 1x1 kernel takes from its epilogue (`kernels.conv(..., chan_sum_out=True)`).

Bounds.  Both new paths compute the same products as the launches they replace; only the grouping of the fp32 sums differs.
So each is measured against a float64 restatement NEXT TO the path it replaces (conv -> gram_partial + chan_sum_partial), and
may show at most 4 x that path's error (regrouped fp32 sums of ~1e5 terms move by a few ulp sqrt(n)).  What is compared is what
the consumer (align_fold / vec_mlp) uses: the cosines G / (|q| |k|), absolute, and the channel means relative to max |mean|.

Measured on MI355X (cosines abs / means rel; existing path -> one-pass kernel), float64 restatement as the reference:
    3x272x480            1.06e-07 / 4.43e-07  ->  1.07e-07 / 3.97e-07
    5x72x120             1.99e-07 / 1.30e-07  ->  2.04e-07 / 2.64e-07
    1x64x64              2.76e-07 / 1.42e-07  ->  2.71e-07 / 2.09e-07
    24x40x56             4.14e-07 / 1.76e-07  ->  4.14e-07 / 1.58e-07
    2x37x53 (ragged)     3.73e-07 / 1.63e-07  ->  3.70e-07 / 1.57e-07
    3x48x80 (slices)     3.25e-07 / 1.42e-07  ->  3.27e-07 / 2.20e-07
(the cosines' error is the split-bf16 product's own error in kf, the same in both paths).  The stream kernel's channel sums, means rel,
chan_sum_partial(out) -> epilogue: 1.50e-07 -> 1.45e-07 (520x8x12), 8.03e-08 -> 1.13e-07 (24x40x56), 2.91e-07 -> 2.40e-07 (3x272x480),
1.11e-07 -> 9.92e-08 (2x37x53).  Forward with the switch off / on: out differs by 6.0e-06 .. 7.3e-06 max-abs, L1_fea by 0.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _operands(B, H, W, seed, sliced=False):
    """warped, pred, q [B,H,W,64] (seeded on the CPU: the same bits in every process) and the packed 128 -> 64 convolution.
    sliced: the three are channel slices of wider tensors (pitch 128 / 192), as `_rdab` hands out xq[..., 64:128]."""
    from cdfo_amd import kernels as K
    g = torch.Generator().manual_seed(seed)
    wide = torch.randn(B, H, W, 192, generator=g) * torch.linspace(0.5, 2.0, 192) + 0.25
    wt = torch.randn(64, 128, 1, 1, generator=g) / 128 ** 0.5
    wide, wt = wide.cuda(), wt.cuda()
    if sliced:
        other = torch.randn(B, H, W, 128, generator=g).cuda()
        x0, x1, q = wide[..., 64:128], other[..., 64:128], wide[..., 128:192]
    else:
        x0, x1, q = (wide[..., i * 64:(i + 1) * 64].contiguous() for i in range(3))
    return x0, x1, q, wt, K.pack_conv(wt, None)


def _fold_sum(part):
    """the consumer's reduction: partials added in index order, fp32"""
    s = torch.zeros_like(part[:, 0])
    for ch in range(part.shape[1]):
        s = s + part[:, ch]
    return s


def _consumed(gram, s0, s1, P, CH=16):
    """(cosines [B,64,CH], means [B,2,64]) in float64 from fp32 partials summed the way the fold kernel sums them"""
    g = _fold_sum(gram).double().view(-1, 64, CH + 2)
    nq = g[:, :, CH].sqrt().clamp_min(1e-12)
    nk = g[:, :, CH + 1].sqrt().clamp_min(1e-12).view(-1, 64 // CH, 1, CH)
    cos = g[:, :, :CH].view(-1, 64 // CH, CH, CH) / (nq.view(-1, 64 // CH, CH, 1) * nk)
    return cos.reshape(-1, 64, CH), torch.stack([_fold_sum(s0), _fold_sum(s1)], 1).double() / P


def _restatement(x0, x1, q, wt, CH=16):
    B = x0.shape[0]
    x = torch.cat([x0, x1], -1).double().view(B, -1, 128)
    kf = torch.relu(x @ wt.double().view(64, 128).t())
    qd = q.double().reshape(B, -1, 64)
    G = torch.einsum("bphc,bphj->bhcj", qd.view(B, -1, 64 // CH, CH), kf.view(B, -1, 64 // CH, CH))
    nq = qd.pow(2).sum(1).sqrt().view(B, 64 // CH, CH, 1)
    nk = kf.pow(2).sum(1).sqrt().view(B, 64 // CH, 1, CH)
    means = torch.stack([x0.double().reshape(B, -1, 64).mean(1), x1.double().reshape(B, -1, 64).mean(1)], 1)
    return (G / (nq * nk)).reshape(B, 64, CH), means


def _errors(got, ref):
    return (got[0] - ref[0]).abs().max().item(), ((got[1] - ref[1]).abs().max() / ref[1].abs().max()).item()


def _le(err, bound, what):
    """the error-against-bound assertions of the persistent kernels' tests (tests/test_gpu_schedules.py records the ratios it sees
    when it re-runs them under a CU limit)"""
    assert err <= bound, f"{what}: {err} (bound {bound})"


@pytest.mark.parametrize("B,H,W,sliced", [(3, 272, 480, False), (5, 72, 120, False), (1, 64, 64, False), (24, 40, 56, False),
                                          (2, 37, 53, False), (3, 48, 80, True)])
def test_align_stats_against_float64(B, H, W, sliced):
    from cdfo_amd import kernels as K
    x0, x1, q, wt, pc = _operands(B, H, W, 1000 + B * H, sliced)
    ref = _restatement(x0, x1, q, wt)
    kf = K.conv([x0, x1], pc, act=K.ACT_RELU, prec=K.PREC_BF16X3)          # the path this kernel replaces
    gp, _ = K.gram_partial(q, kf, 16)
    old = _errors(_consumed(gp, K.chan_sum_partial(x0)[0], K.chan_sum_partial(x1)[0], H * W), ref)
    gram, s0, s1, n = K.align_stats(x0, x1, q, pc, K.ACT_RELU, 16)
    assert gram.shape == (B, n, 64 * 18) and s0.shape == s1.shape == (B, n, 64)
    new = _errors(_consumed(gram, s0, s1, H * W), ref)
    torch.cuda.synchronize()
    print(f"align_stats {B}x{H}x{W}{' sliced' if sliced else ''}: cosines abs {old[0]:.2e} -> {new[0]:.2e}, "
          f"means rel {old[1]:.2e} -> {new[1]:.2e}, slots {n}")
    _le(new[0], 4 * old[0], f"align_stats cosines {(old, new)}")
    _le(new[1], 4 * old[1], f"align_stats means {(old, new)}")


@pytest.mark.parametrize("B,H,W,nsrc", [(520, 8, 12, 3), (24, 40, 56, 3), (3, 272, 480, 3), (2, 37, 53, 1)])
def test_stream_kernel_channel_sums(B, H, W, nsrc):
    """chan_sum_out against chan_sum_partial(out) of the same call: same result tensor, sums equal to within regrouping (the 4 x rule
    against float64).  520x8x12: 96-pixel images (a ragged tile each), two and more images per workgroup; 2x37x53: ragged last tile."""
    from cdfo_amd import kernels as K
    g = torch.Generator().manual_seed(7 * B + H)
    srcs = [(torch.randn(B, H, W, 64, generator=g) + 0.3).cuda() for _ in range(nsrc)]
    if nsrc == 3:     # per-image weights, as the folded alignment convolution
        pc = K.PackedConv((torch.randn(B, 192 * 64, generator=g) / 192 ** 0.5).cuda(), None, 64, 192, 1, 64, False, 192 * 64)
    else:
        pc = K.pack_conv((torch.randn(64, 64, 1, 1, generator=g) / 8).cuda(), (torch.randn(64, generator=g) * 0.1).cuda())
    out, part, n = K.conv(srcs, pc, act=K.ACT_RELU, prec=K.PREC_BF16X3, chan_sum_out=True)
    assert part.shape == (B, n, 64)
    plain = K.conv(srcs, pc, act=K.ACT_RELU, prec=K.PREC_BF16X3)
    assert torch.equal(out, plain)                                           # the result itself is untouched by the extra output
    ref = out.double().view(B, -1, 64).mean(1)
    scale = ref.abs().max()
    old = ((_fold_sum(K.chan_sum_partial(out)[0]).double() / (H * W) - ref).abs().max() / scale).item()
    new = ((_fold_sum(part).double() / (H * W) - ref).abs().max() / scale).item()
    torch.cuda.synchronize()
    print(f"chan_sum_out {B}x{H}x{W}: means rel {old:.2e} -> {new:.2e}, slots {n}")
    _le(new, 4 * old, f"chan_sum_out means {(old, new)}")


def _dump(path):
    """the partials of one seeded call -> path (also run in a second process by the test below)"""
    from cdfo_amd import kernels as K
    x0, x1, q, _, pc = _operands(5, 72, 120, 4242)
    gram, s0, s1, _ = K.align_stats(x0, x1, q, pc, K.ACT_RELU, 16)
    fold = K.PackedConv((torch.randn(5, 192 * 64, generator=torch.Generator().manual_seed(5)) / 14).cuda(), None, 64, 192, 1, 64, False, 192 * 64)
    _, part, _ = K.conv([x0, x1, q], fold, act=K.ACT_RELU, prec=K.PREC_BF16X3, chan_sum_out=True)
    torch.cuda.synchronize()
    arrs = [t.cpu().numpy() for t in (gram, s0, s1, part)]
    if path:
        np.savez(path, *arrs)
    return arrs


def test_partials_are_bitwise_reproducible(tmp_path):
    from conftest import clean_process_run
    first, second = _dump(None), _dump(None)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    path = str(tmp_path / "partials.npz")
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_gpu_align_stats as t; t._dump({path!r})"
    rc, so, se = clean_process_run([sys.executable, "-c", code], cwd=ROOT, timeout=120)
    assert rc == 0, se[-2000:]
    other = np.load(path)
    for i, a in enumerate(first):
        assert a.tobytes() == other[f"arr_{i}"].tobytes(), i


@pytest.mark.parametrize("B,H,W,seed", [(1, 24, 40, None), (1, 64, 64, 910), (3, 272, 480, 911)])
def test_forward_with_and_without_the_fused_statistics(B, H, W, seed):
    """model.align_stats (CDFO_ALIGN_STATS) off and on: the same forward up to reordered fp32 sums in 70 K statistics per image.
    Bound: a tenth of the forward's parity bound (1e-3); the first case is the 24x40 golden and is also held to the golden itself."""
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
            m.align_stats = on
            out, l1 = m(dev["x"], dev["mvs0"], dev["mvs1"], dev["pms"], dev["rms"], dev["ufs"], gumbel_uniform=noise)
            res[on] = (out.clone(), l1.clone())
    torch.cuda.synchronize()
    d_out = (res[True][0] - res[False][0]).abs().max().item()
    d_l1 = (res[True][1] - res[False][1]).abs().max().item()
    print(f"align_stats off/on {B}x{H}x{W}: out {d_out:.2e} L1_fea {d_l1:.2e}")
    assert d_out <= 1e-4 and d_l1 <= 1e-4
    if gold is not None:
        assert (res[True][0].cpu() - torch.from_numpy(gold["out"])).abs().max().item() <= 1e-3
