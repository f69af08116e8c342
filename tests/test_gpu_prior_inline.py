"""The plane chunk of the stream kernels (csrc/plane_chunk.h): a 64-channel operand that is a 3x3 stencil of a one-channel plane joins a
1x1 product as one more k-step of 16, built in registers from the plane; the operand itself is never written.  Against the launches it
replaces: `stem_conv` (which writes the operand, or its sum with the features) followed by the same consumer.

    conv (streaming 1x1)   residual form: RDAB.fuse with res1 = fea_com = fea + conv_expand_rms(rms)  ->  res1 = fea + the chunk;
                           K-block form with per-image weights and the channel sums of the result (the folded convolution of the
                           alignment: [x0, stencil, x2] 192 -> 64 + ReLU)  ->  [x0, x2] + the chunk
    rdab_prep_fused        input_conv on fea_com  ->  on fea + the chunk

Bounds.  Both paths end in the same split-bf16 product (hi*lo + lo*hi + hi*hi, fp32 accumulation).  The replaced path forms the stencil
with nine fp32 FMAs and splits the SUM; the chunk splits the nine neighbours and the composed weights, one more product of the same
kind.  So each is measured against a float64 restatement (shifted products, no library convolution) NEXT TO the other on the same
inputs, and the new path may show at most 4 x the replaced path's error (the rule of tests/test_gpu_align_stats.py and
test_gpu_rdab_stats.py).  Compared is what the consumer uses, relative to max |reference|: the stream kernel's output and channel
sums; sq, vrow, qwin, vwin.  The mask (qwin == 0) depends on vmax and the draws alone: torch.equal.  fp16 V outputs: the fp32
variant rounded once, torch.equal.  The planes are slots of a [B,1,7,H,W] stack whose other slots hold 100: a read across a plane's
end shows as an error of that size.

Measured on MI355X (replaced path -> plane chunk; error relative to max |reference|), float64 restatement as the reference:
    conv, residual form       2x8x8 3.18e-06 -> 3.19e-06;  1x16x24 3.22e-06 -> 3.21e-06;  1x64x2 3.61e-06 -> 3.56e-06;
                              1x2x64 3.03e-06 -> 3.08e-06;  1x24x40 4.16e-06 -> 4.16e-06;  3x6x10 3.48e-06 -> 3.50e-06;
                              3x2x8x8 through the strides 3.43e-06 -> 3.28e-06;  5x16x24 on 1 / 4 / 7 CUs 3.81e-06 -> 3.92e-06
    conv, K block (out / sums) 2x8x8 5.25e-06 / 2.22e-06 -> 5.10e-06 / 2.08e-06;  1x16x24 4.89e-06 / 8.88e-07 -> 4.95e-06 / 1.67e-06;
                              1x64x2 5.42e-06 / 1.23e-06 -> 5.50e-06 / 1.34e-06;  1x2x64 4.95e-06 / 1.32e-06 -> 5.02e-06 / 1.65e-06;
                              1x24x40 5.04e-06 / 9.69e-07 -> 4.97e-06 / 9.69e-07;  3x6x10 4.55e-06 / 1.85e-06 -> 4.73e-06 / 1.66e-06;
                              5x16x24 on 1 / 4 / 7 CUs 4.94e-06 / 1.51e-06 -> 4.98e-06 / 1.25e-06, 1.18e-06, 1.24e-06
    mask kernel (sq, vrow,    2x8x8 4.42e-06, 5.05e-06, 7.28e-06, 5.58e-06 -> 3.82e-06, 4.77e-06, 5.37e-06, 4.25e-06
    qwin, vwin)               1x16x24 6.66e-06, 5.43e-06, 5.11e-06, 4.67e-06 -> 4.83e-06, 5.08e-06, 4.77e-06, 5.27e-06
                              1x64x2 2.46e-06, 3.22e-06, 4.70e-06, 5.38e-06 -> 3.56e-06, 3.82e-06, 5.23e-06, 5.25e-06
                              1x2x64 3.97e-06, 4.37e-06, 5.16e-06, 5.48e-06 -> 6.73e-06, 4.91e-06, 5.65e-06, 6.08e-06
                              1x24x40 4.25e-06, 5.02e-06, 5.66e-06, 5.65e-06 -> 4.99e-06, 4.30e-06, 5.33e-06, 5.25e-06
                              3x2x8x8 through the strides 3.78e-06, 4.17e-06, 4.84e-06, 5.83e-06 -> 2.99e-06, 5.51e-06, 4.99e-06, 6.24e-06
                              5x16x24 on 1 / 4 / 7 CUs 3.75e-06, 3.53e-06, 5.04e-06, 5.93e-06 -> 3.33e-06, 3.42e-06, 5.57e-06, 5.15e-06
(the largest ratio new / old is 1.9, the channel sums at 1x16x24; the bound is 4).  Forward with model.inline_rms off / on, injected noise:
L1_fea identical, out differs by 8.05e-06 (24x40 golden) and 5.99e-06 (1x64x64); stem_conv launches per forward 13 -> 7.
"""
import os
import sys

import numpy as np
import pytest
import torch

import attn_cases as AC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the smallest shapes at which the tap fetch can go wrong: P = 64 is half a tile (waves beyond the image); a wave's 32 pixels span two
# rows (W = 24); every pixel on a border (W = 2, H = 2); 7.5 tiles; P = 60 (stream kernel only: the mask kernel needs P % 64 == 0)
SHAPES = [(2, 8, 8), (1, 16, 24), (1, 64, 2), (1, 2, 64), (1, 24, 40)]
STREAM_SHAPES = SHAPES + [(3, 6, 10)]


def _stencil_weights(seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(64, 1, 3, 3, generator=g) / 3).cuda(), (torch.randn(64, generator=g) * 0.1).cuda()


def _stack(B, H, W, seed, slots):
    """[B,1,7,H,W]: the `slots` hold residual maps (signed, a third of the samples zero), every other slot 100"""
    g = torch.Generator().manual_seed(seed)
    m = torch.full((B, 1, 7, H, W), 100.0)
    for i in slots:
        m[:, 0, i] = torch.randn(B, H, W, generator=g) * 0.2 * (torch.rand(B, H, W, generator=g) > 0.33)
    return m.cuda()


def _stencil64(planes, w, b):
    """float64: planes [M,H,W] -> stencil9(plane; w, b) [M,H,W,64], zero padding, as shifted products"""
    M, H, W = planes.shape
    x = torch.zeros(M, H + 2, W + 2, dtype=torch.float64, device=planes.device)
    x[:, 1:-1, 1:-1] = planes.double()
    out = b.double().view(1, 1, 1, 64).repeat(M, H, W, 1)
    for u in range(9):
        out += x[:, u // 3:u // 3 + H, u % 3:u % 3 + W, None] * w.double().view(64, 9)[:, u]
    return out


def _chanconv64(x, w9, b):
    """float64 zero-padded 9-tap cross-correlation along the channel axis (arch.py:2216-2219) as shifted products"""
    out = torch.full_like(x, float(b))
    for t in range(9):
        lo, hi = max(0, 4 - t), min(64, 68 - t)
        out[..., lo:hi] += float(w9[t]) * x[..., lo + t - 4:hi + t - 4]
    return out


def _rel(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


def _fold(part):
    s = torch.zeros_like(part[:, 0])
    for k in range(part.shape[1]):
        s = s + part[:, k]
    return s.double()


def _views(stack, slots):
    """the group's addressing: images slot major, image m's plane at view + (m % B) 7 P + (m // B) P"""
    B, _, _, H, W = stack.shape
    return [stack[:, 0, i] for i in slots], (stack[:, 0, slots[0]], B, 7 * H * W, H * W if len(slots) > 1 else 0)


# ----------------------------------------------------------------------------------------------------------- the stream kernel
def _residual_case(B, H, W, slots, seed):
    """RDAB.fuse: out = fuse(cat) + (fea + stencil).  Returns (old error, new error)"""
    from cdfo_amd import kernels as K
    stack = _stack(B, H, W, seed, slots)
    views, addr = _views(stack, slots)
    M, P = B * len(slots), H * W
    g = torch.Generator().manual_seed(seed + 1)
    cat, fea = torch.randn(M, H, W, 128, generator=g).cuda(), torch.randn(M, H, W, 64, generator=g).cuda()
    wf, bf = (torch.randn(64, 128, 1, 1, generator=g) / 11).cuda(), (torch.randn(64, generator=g) * 0.1).cuda()
    ws, bs = _stencil_weights(seed + 2)
    pc = K.pack_conv(wf, bf)
    ref = cat.double() @ wf.double().view(64, 128).t() + bf.double() + fea.double() + _stencil64(torch.cat(views, 0), ws, bs)
    fea_com = torch.empty_like(fea)
    for n, v in enumerate(views):
        K.stem_conv(v, 7 * P, B, H, W, ws, bs, add=fea[n * B:(n + 1) * B], out2=fea_com[n * B:(n + 1) * B], write_out=False)
    old = K.conv(cat, pc, res1=fea_com, prec=K.PREC_FP16X2)
    new = K.conv(cat, pc, res1=fea, prec=K.PREC_FP16X2, plane=(*addr, K.pack_plane_chunk(ws, bs)))
    torch.cuda.synchronize()
    return _rel(old, ref), _rel(new, ref)


def _kblock_case(B, H, W, slots, seed, want=False):
    """the folded convolution's form: relu(W_b . [x0; stencil; x2] + bias) with per-image weights, and the result's channel sums.
    Returns ((old out, old sums), (new out, new sums)) errors, or with `want` the new path's (out, partials)"""
    from cdfo_amd import kernels as K
    stack = _stack(B, H, W, seed, slots)
    views, addr = _views(stack, slots)
    M, P = B * len(slots), H * W
    g = torch.Generator().manual_seed(seed + 1)
    x0, x2 = torch.randn(M, H, W, 64, generator=g).cuda(), torch.randn(M, H, W, 64, generator=g).cuda()
    wb = (torch.randn(M, 64, 192, generator=g) / 13).cuda()
    bias = (torch.randn(64, generator=g) * 0.1).cuda()
    ws, bs = _stencil_weights(seed + 2)
    pk = lambda w: torch.cat([K.pack_conv(w[m].reshape(64, -1, 1, 1).contiguous(), None).w for m in range(M)])
    pc192 = K.PackedConv(pk(wb), bias, 64, 192, 1, 64, w_bstride=192 * 64)
    pc128 = K.PackedConv(pk(torch.cat([wb[:, :, :64], wb[:, :, 128:]], 2)), bias, 64, 128, 1, 64, w_bstride=128 * 64)
    zero = torch.zeros(64, device="cuda")
    tables = torch.stack([K.pack_plane_chunk(*K.compose_stem_1x1(ws, bs, wb[m, :, 64:128].reshape(64, 64, 1, 1), zero))
                          for m in range(M)]).contiguous()
    new = K.conv([x0, x2], pc128, act=K.ACT_RELU, prec=K.PREC_FP16X2, chan_sum_out=True, plane=(*addr, tables, 64 * 16))
    if want:
        torch.cuda.synchronize()
        return new[0], new[1]
    pred = torch.empty_like(x0)
    for n, v in enumerate(views):
        K.stem_conv(v, 7 * P, B, H, W, ws, bs, out=pred[n * B:(n + 1) * B])
    old = K.conv([x0, pred, x2], pc192, act=K.ACT_RELU, prec=K.PREC_FP16X2, chan_sum_out=True)
    st = _stencil64(torch.cat(views, 0), ws, bs)
    ref = torch.relu(torch.einsum("mhwc,moc->mhwo", torch.cat([x0.double(), st, x2.double()], 3), wb.double()) + bias.double())
    rsum = ref.sum((1, 2))
    torch.cuda.synchronize()
    assert new[2] == old[2] and new[1].shape == old[1].shape
    return ((_rel(old[0], ref), _rel(_fold(old[1]), rsum)), (_rel(new[0], ref), _rel(_fold(new[1]), rsum)))


@pytest.mark.parametrize("B,H,W", STREAM_SHAPES)
def test_stream_kernel_with_the_plane_as_part_of_the_residual(B, H, W):
    old, new = _residual_case(B, H, W, [3], 500 + H)
    print(f"plane chunk, conv residual {B}x{H}x{W}: out rel {old:.2e} -> {new:.2e}")
    assert new <= 4 * old, (old, new)


@pytest.mark.parametrize("B,H,W", STREAM_SHAPES)
def test_stream_kernel_with_the_plane_as_a_k_block_per_image_weights_and_channel_sums(B, H, W):
    old, new = _kblock_case(B, H, W, [3], 600 + H)
    print(f"plane chunk, conv K block {B}x{H}x{W}: out rel {old[0]:.2e} -> {new[0]:.2e}, sums rel {old[1]:.2e} -> {new[1]:.2e}")
    assert new[0] <= 4 * old[0] and new[1] <= 4 * old[1], (old, new)


def test_stream_kernel_group_through_the_plane_strides():
    """6 images as 3 slots x 2 windows in ONE launch; the last slots of the stack, so that a stride error reads beyond it"""
    old, new = _residual_case(2, 8, 8, [4, 5, 6], 77)
    ko, kn = _kblock_case(2, 8, 8, [4, 5, 6], 78)
    print(f"plane chunk, conv 3x2x8x8 strided: residual {old:.2e} -> {new:.2e}, K block {ko[0]:.2e} -> {kn[0]:.2e}, sums {ko[1]:.2e} -> {kn[1]:.2e}")
    assert new <= 4 * old and kn[0] <= 4 * ko[0] and kn[1] <= 4 * ko[1]


@pytest.mark.parametrize("cus", [1, 4, 7])
def test_stream_kernel_with_many_tiles_per_workgroup(cus):
    """5 x 16 x 24 = 15 tiles on 1, 4 and 7 workgroups: several tiles per ring, tap slots reused, segments crossing images"""
    from cdfo_amd import kernels as K
    with K.cu_limit(cus):
        old, new = _residual_case(5, 16, 24, [3], 900)
        ko, kn = _kblock_case(5, 16, 24, [3], 901)
    print(f"plane chunk, conv 5x16x24 on {cus} CUs: residual {old:.2e} -> {new:.2e}, K block {ko[0]:.2e} -> {kn[0]:.2e}, sums {ko[1]:.2e} -> {kn[1]:.2e}")
    assert new <= 4 * old and kn[0] <= 4 * ko[0] and kn[1] <= 4 * ko[1]


# ----------------------------------------------------------------------------------------------------------- the mask kernel
@pytest.fixture(scope="module")
def input_conv():
    g = torch.Generator().manual_seed(64128)
    return (torch.randn(128, 64, 1, 1, generator=g) / 8.0).cuda(), (torch.randn(128, generator=g) * 0.1).cuda()


def _mask_case(B, H, W, slots, seed, input_conv, want=False):
    from cdfo_amd import kernels as K
    wt, bt = input_conv
    pc = K.pack_conv(wt, bt)
    stack = _stack(B, H, W, seed, slots)
    views, addr = _views(stack, slots)
    M, P = B * len(slots), H * W
    _, vmax, u, wW, bW = (t.cuda() for t in AC.rdab_inputs(M, H, W))
    fea = torch.randn(M, H, W, 64, generator=torch.Generator().manual_seed(seed + 1)).cuda()
    ws, bs = _stencil_weights(seed + 2)
    table = K.pack_plane_chunk(*K.compose_stem_1x1(ws, bs, wt, torch.zeros_like(bt)))
    new = K.rdab_prep_fused(fea, pc, vmax, u, wW, bW, v_f16=False, plane=(*addr, table))
    if want:
        torch.cuda.synchronize()
        return new
    new16 = K.rdab_prep_fused(fea, pc, vmax, u, wW, bW, v_f16=True, plane=(*addr, table))
    fea_com = torch.empty_like(fea)
    for n, v in enumerate(views):
        K.stem_conv(v, 7 * P, B, H, W, ws, bs, add=fea[n * B:(n + 1) * B], out2=fea_com[n * B:(n + 1) * B], write_out=False)
    old = K.rdab_prep_fused(fea_com, pc, vmax, u, wW, bW, v_f16=False)
    torch.cuda.synchronize()
    # float64: the mask is the replaced path's (it depends on vmax and the draws alone; equality is asserted on its own)
    xq = (fea.double() + _stencil64(torch.cat(views, 0), ws, bs)) @ wt.double().view(128, 64).t() + bt.double()
    q, v = xq[..., :64], xq[..., 64:]
    mask = (old[2] == 0).double()
    w9 = wW.double().reshape(-1)
    ref = (_chanconv64(mask * q, w9, bW.double()), _chanconv64(v, w9, bW.double()), (1.0 - mask) * q, v)
    assert torch.equal(new[2] == 0, old[2] == 0) and torch.equal(new16[2] == 0, old[2] == 0)           # the mask, no element excluded
    assert torch.equal(new16[0], new[0]) and torch.equal(new16[2], new[2])
    assert torch.equal(new16[1], new[1].half()) and torch.equal(new16[3], new[3].half())                # fp16 V: rounded once
    return [_rel(o, r) for o, r in zip(old, ref)], [_rel(o, r) for o, r in zip(new, ref)]


def _report(tag, old, new):
    print(f"plane chunk, mask kernel {tag}: " + ", ".join(f"{n} {o:.2e} -> {w:.2e}" for n, o, w in zip(("sq", "vrow", "qwin", "vwin"), old, new)))
    for o, w in zip(old, new):
        assert w <= 4 * o, (old, new)


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_mask_kernel_on_fea_and_the_plane(B, H, W, input_conv):
    _report(f"{B}x{H}x{W}", *_mask_case(B, H, W, [3], 700 + H, input_conv))


def test_mask_kernel_group_through_the_plane_strides(input_conv):
    _report("3x2x8x8 strided", *_mask_case(2, 8, 8, [4, 5, 6], 79, input_conv))


@pytest.mark.parametrize("cus", [1, 4, 7])
def test_mask_kernel_with_many_tiles_per_workgroup(cus, input_conv):
    from cdfo_amd import kernels as K
    with K.cu_limit(cus):
        res = _mask_case(5, 16, 24, [3], 902, input_conv)
    _report(f"5x16x24 on {cus} CUs", *res)


# ----------------------------------------------------------------------------------------------------------- determinism
def _dump(path):
    """the outputs and partials of one seeded call of each kernel (several tiles per workgroup segment) -> path"""
    g = torch.Generator().manual_seed(64128)
    ic = ((torch.randn(128, 64, 1, 1, generator=g) / 8.0).cuda(), (torch.randn(128, generator=g) * 0.1).cuda())
    out, part = _kblock_case(5, 16, 24, [1, 2], 4242, want=True)
    sq, vrow, qwin, vwin = _mask_case(5, 16, 24, [1, 2], 4243, ic, want=True)
    arrs = {k: v.cpu().numpy() for k, v in dict(out=out, part=part, sq=sq, vrow=vrow, qwin=qwin, vwin=vwin).items()}
    if path:
        np.savez(path, **arrs)
    return arrs


def test_results_are_bitwise_reproducible(tmp_path):
    from conftest import clean_process_run
    first, second = _dump(None), _dump(None)
    assert all(first[k].tobytes() == second[k].tobytes() for k in first)
    path = str(tmp_path / "dump.npz")
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_gpu_prior_inline as t; t._dump({path!r})"
    rc, so, se = clean_process_run([sys.executable, "-c", code], cwd=ROOT, timeout=120)
    assert rc == 0, se[-2000:]
    other = np.load(path)
    assert all(first[k].tobytes() == other[k].tobytes() for k in first)


# ----------------------------------------------------------------------------------------------------------- the model
def _model(wseed):
    from arch.SIDECVSR_our import CVSR_V8
    from oracle.cvsr_v8_ref import make_state_dict
    m = CVSR_V8()
    m.load_state_dict(make_state_dict(wseed), strict=True)
    return m.cuda().eval()


@pytest.mark.parametrize("B,H,W,seed", [(1, 24, 40, None), (1, 64, 64, 910)])
def test_forward_with_and_without_inline_rms(B, H, W, seed):
    """model.inline_rms (CDFO_INLINE_RMS) off and on, injected noise: L1_fea identical (the neighbour phase does not reach it), out
    within a tenth of the forward's parity bound; the first case is the 24x40 golden and is also held to the golden."""
    from oracle.cvsr_v8_ref import make_inputs
    gold = None
    if seed is None:
        gold = np.load(os.path.join(ROOT, "tests", "golden", "cvsr_v8_b1_24x40.npz"))
        wseed, seed, layout = int(gold["wseed"]), int(gold["iseed"]), str(gold["layout"])
    else:
        wseed, layout = 21, "b1n"
    m = _model(wseed)
    inp = make_inputs(B, H, W, seed, layout)
    dev = {k: v.cuda() for k, v in inp.items() if k != "gumbel_u"}
    noise = [u.cuda() for u in inp["gumbel_u"]]
    res, calls = {}, {}
    from cdfo_amd import kernels as K
    real = K.stem_conv
    with torch.no_grad():
        for on in (False, True):
            m.inline_rms = on
            n = [0]

            def counted(*a, **kw):
                n[0] += 1
                return real(*a, **kw)
            K.stem_conv = counted
            try:
                out, l1 = m(dev["x"], dev["mvs0"], dev["mvs1"], dev["pms"], dev["rms"], dev["ufs"], gumbel_uniform=noise)
            finally:
                K.stem_conv = real
            res[on], calls[on] = (out.clone(), l1.clone()), n[0]
    torch.cuda.synchronize()
    d_out = (res[True][0] - res[False][0]).abs().max().item()
    print(f"inline_rms off/on {B}x{H}x{W}: out {d_out:.2e}, stem_conv launches {calls[False]} -> {calls[True]}")
    assert calls[False] - calls[True] == 6          # the six fea_com stems of a forward
    assert torch.equal(res[True][1], res[False][1])
    assert d_out <= 1e-4
    if gold is not None:
        assert (res[True][0].cpu() - torch.from_numpy(gold["out"])).abs().max().item() <= 1e-3


def test_non_affine_stems_take_the_materialised_path():
    """stems on the slots 1, 3, 6 (no common stride): `_compensate` writes fea_com as with the switch off -- same bits"""
    m = _model(21)
    B, H, W = 1, 16, 24
    w = m._weights()
    rms = _stack(B, H, W, 31, [1, 2, 3, 6])
    fea = torch.randn(3 * B, H, W, 64, generator=torch.Generator().manual_seed(5)).cuda()
    noise = [AC.rdab_inputs(B, H, W, seed=s)[2].cuda() for s in range(3)]
    stems = [(rms[:, 0, i], 7 * H * W, slice(n * B, (n + 1) * B)) for n, i in enumerate((1, 3, 6))]
    assert m._inline_rms_planes(w, fea, stems, 3) is None
    assert m._inline_rms_planes(w, fea, [(rms[:, 0, i], 7 * H * W, slice(n * B, (n + 1) * B)) for n, i in enumerate((1, 2, 3))], 3) is not None
    res = {}
    with torch.no_grad():
        for on in (False, True):
            m.inline_rms = on
            res[on] = [t.clone() for t in m._compensate(w, fea, stems, [0, 1, 2], noise)]
    torch.cuda.synchronize()
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])


def test_compensate_features_does_not_depend_on_the_frames_sharing_the_call():
    """compensate_features has ONE stem for its F frames and a noise per frame: a frame's result carries the same bits whether it
    comes alone or with three others (the chunked evaluators rely on it), so both forms must take the same path."""
    m = _model(21)
    F, H, W = 4, 16, 24
    g = torch.Generator().manual_seed(8)
    fea = torch.randn(F, H, W, 64, generator=g).cuda()
    rms = torch.rand(F, 1, H, W, generator=g).cuda()
    noise = [AC.rdab_inputs(1, H, W, seed=s)[2].cuda() for s in range(F)]
    with torch.no_grad():
        together = m.compensate_features(fea, rms, gumbel_uniform=noise).clone()
        alone = [m.compensate_features(fea[f:f + 1].contiguous(), rms[f:f + 1].contiguous(), gumbel_uniform=[noise[f]]).clone() for f in range(F)]
    torch.cuda.synchronize()
    assert torch.equal(together, torch.cat(alone, 0))
