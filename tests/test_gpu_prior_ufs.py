"""`model.inline_ufs` (CDFO_INLINE_UFS): ufs_prior = conv_expand_ufs(ufs) never reaches memory.  Its two readers take it as the plane chunk
of their products (csrc/plane_chunk.h): the statistics pass of DualAttAlignment (`kernels.align_stats(..., plane=)`, the `PLANE` form of
align_gram_partial_kernel) and the folded convolution (`kernels.conv(..., plane=)` with the per-image tables of
`kernels.align_fold_plane`; that kernel form is tested in test_gpu_prior_inline.py).  Against the launches they replace: `stem_conv`
(which writes ufs_prior) followed by `align_stats` / `align_fold`.

Bounds.  The statistics kernel: kf = relu(Wf . [x0; stencil] + bias) ends in the same split-bf16 product on both paths; the replaced
path forms the stencil with nine fp32 FMAs and splits the sum, the chunk splits the nine neighbours and the composed weights.  The
channel sums of the stencil come from 64-channel values on the replaced path and from the plane's ten tap sums on the new one.  Each
path is measured against a float64 restatement NEXT TO the other on the same inputs, and the new one may show at most 4 x the replaced
path's error (the rule of test_gpu_align_stats.py, test_gpu_rdab_stats.py and test_gpu_prior_inline.py).  Compared is what the consumer
(align_fold) uses: the cosines G / (|q| |kf|), absolute; the channel means of x0 and of the stencil, each relative to its max |mean|.
The composition: [M1 | Wb] `torch.equal` to align_fold's columns; the tables against float64 M2 @ [w_u | b_u] from that same output,
at most 4 x the error of the fp32 product (i ascending).  The planes are slots of a [B,1,7,H,W] stack whose other slots hold 100: a
read across a plane's end shows as an error of that size.

Measured on MI355X (replaced path -> plane form; cosines abs / means of the stencil rel; the sums of x0 are bit-equal on both paths,
5.0e-08 .. 1.8e-07), float64 restatement as the reference:
    2x8x8      2.10e-06 / 4.45e-08 -> 2.14e-06 / 3.19e-08        1x16x24    8.73e-07 / 4.72e-08 -> 8.23e-07 / 4.17e-08
    1x64x2     1.48e-06 / 5.92e-08 -> 1.65e-06 / 4.80e-08        1x2x64     1.53e-06 / 7.36e-08 -> 1.45e-06 / 4.17e-08
    1x24x40    5.36e-07 / 6.46e-08 -> 5.33e-07 / 6.46e-08        3x6x10     3.25e-06 / 7.23e-08 -> 3.05e-06 / 3.20e-08
    2x37x53    3.69e-07 / 7.72e-08 -> 3.86e-07 / 7.73e-08        3x2x8x8 through the strides 2.62e-06 / 8.02e-08 -> 2.38e-06 / 3.57e-08
    5x16x24 on 1 / 4 / 7 CUs  8.70e-07 / 5.71e-08 -> 9.07e-07 / 3.66e-08,  8.67e-07 / 5.26e-08 -> 9.11e-07 / 3.66e-08,
                              8.63e-07 / 6.80e-08 -> 9.09e-07 / 5.21e-08
    1x16x24, 8 channels per head  7.91e-07 / 5.82e-08 -> 7.76e-07 / 5.40e-08
(the largest ratio new / old is 1.11, the cosines at 1x64x2; the bound is 4).  The fold's tables, fp32 product -> align_fold_plane
(double accumulation, rounded once): 2.86e-07 -> 3.42e-08 (2x8x8), 2.15e-07 -> 3.49e-08 (5x16x24).  Forward with model.inline_ufs off /
on, injected noise: L1_fea identical, out differs by 7.27e-06 (24x40 golden) and 7.33e-06 (1x64x64); stem_conv launches per forward 7 -> 1.
"""
import os
import sys

import numpy as np
import pytest
import torch

import test_gpu_prior_inline as PI

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the smallest shapes at which the tap fetch or the segment logic can go wrong: half a tile (waves beyond the image); a wave's 32
# pixels span two rows; every pixel on a border (twice); 7.5 tiles; ragged P (twice)
SHAPES = [(2, 8, 8), (1, 16, 24), (1, 64, 2), (1, 2, 64), (1, 24, 40), (3, 6, 10), (2, 37, 53)]


def _consumed(gram, s0, s1, P, CH=16):
    """(cosines [M,64,CH], means of x0 [M,64], means of x1 [M,64]) in float64 from fp32 partials summed the way the fold kernel does"""
    g = PI._fold(gram).view(-1, 64, CH + 2)
    nq = g[:, :, CH].sqrt().clamp_min(1e-12)
    nk = g[:, :, CH + 1].sqrt().clamp_min(1e-12).view(-1, 64 // CH, 1, CH)
    cos = g[:, :, :CH].view(-1, 64 // CH, CH, CH) / (nq.view(-1, 64 // CH, CH, 1) * nk)
    return cos.reshape(-1, 64, CH), PI._fold(s0) / P, PI._fold(s1) / P


def _errors(got, ref):
    return ((got[0] - ref[0]).abs().max().item(), ((got[1] - ref[1]).abs().max() / ref[1].abs().max()).item(),
            ((got[2] - ref[2]).abs().max() / ref[2].abs().max()).item())


def _stats_case(B, H, W, slots, seed, want=False, CH=16):
    """stem_conv -> align_stats against align_stats(plane=).  Returns (old errors, new errors), or with `want` the new partials"""
    from cdfo_amd import kernels as K
    stack = PI._stack(B, H, W, seed, slots)
    views, addr = PI._views(stack, slots)
    M, P = B * len(slots), H * W
    g = torch.Generator().manual_seed(seed + 1)
    x0 = (torch.randn(M, H, W, 64, generator=g) * torch.linspace(0.5, 2.0, 64) + 0.25).cuda()
    q = (torch.randn(M, H, W, 64, generator=g) + 0.1).cuda()
    wt, bt = (torch.randn(64, 128, 1, 1, generator=g) / 128 ** 0.5).cuda(), (torch.randn(64, generator=g) * 0.1).cuda()
    ws, bs = PI._stencil_weights(seed + 2)
    pc = K.pack_conv(wt, bt)
    table = K.pack_plane_chunk(*K.compose_stem_1x1(ws, bs, wt[:, 64:], torch.zeros_like(bt)))
    new = K.align_stats(x0, None, q, pc, K.ACT_RELU, CH, plane=(*addr, table, K.pack_plane_chunk(ws, bs)))
    if want:
        torch.cuda.synchronize()
        return new[:3]
    pred = torch.empty_like(x0)
    for n, v in enumerate(views):
        K.stem_conv(v, 7 * P, B, H, W, ws, bs, out=pred[n * B:(n + 1) * B])
    old = K.align_stats(x0, pred, q, pc, K.ACT_RELU, CH)
    # float64 restatement
    st = PI._stencil64(torch.cat(views, 0), ws, bs)
    kf = torch.relu(torch.cat([x0.double(), st], 3).view(M, P, 128) @ wt.double().view(64, 128).t() + bt.double())
    qd = q.double().view(M, P, 64)
    G = torch.einsum("bphc,bphj->bhcj", qd.view(M, P, 64 // CH, CH), kf.view(M, P, 64 // CH, CH))
    nq = qd.pow(2).sum(1).sqrt().view(M, 64 // CH, CH, 1)
    nk = kf.pow(2).sum(1).sqrt().view(M, 64 // CH, 1, CH)
    ref = ((G / (nq * nk)).reshape(M, 64, CH), x0.double().view(M, P, 64).mean(1), st.view(M, P, 64).mean(1))
    torch.cuda.synchronize()
    assert new[3] == old[3] and all(a.shape == b.shape for a, b in zip(new[:3], old[:3]))
    assert torch.equal(new[1], old[1])                      # the sums of x0: the same instructions on the same bytes
    return _errors(_consumed(*old[:3], P, CH), ref), _errors(_consumed(*new[:3], P, CH), ref)


def _report(tag, old, new):
    print(f"align_stats plane {tag}: cosines abs {old[0]:.2e} -> {new[0]:.2e}, means x0 rel {old[1]:.2e} -> {new[1]:.2e}, "
          f"means stencil rel {old[2]:.2e} -> {new[2]:.2e}")
    for o, n, what in zip(old, new, ("cosines", "means of x0", "means of the stencil")):
        assert n <= 4 * o, f"{tag} {what}: {n} (bound 4 x {o})"


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_statistics_kernel_with_the_stencil_as_a_plane(B, H, W):
    _report(f"{B}x{H}x{W}", *_stats_case(B, H, W, [3], 300 + 7 * H + W))


def test_statistics_kernel_group_through_the_plane_strides():
    """6 images as 3 slots x 2 windows in ONE launch; the last slots of the stack, so that a stride error reads beyond it"""
    _report("3x2x8x8 strided", *_stats_case(2, 8, 8, [4, 5, 6], 81))


@pytest.mark.parametrize("cus", [1, 4, 7])
def test_statistics_kernel_with_many_tiles_per_workgroup(cus):
    """5 x 16 x 24 = 15 tiles on 1, 4 and 7 workgroups: several tiles per ring, tap slots reused, segments crossing images"""
    from cdfo_amd import kernels as K
    with K.cu_limit(cus):
        res = _stats_case(5, 16, 24, [3], 903)
    _report(f"5x16x24 on {cus} CUs", *res)


def test_statistics_kernel_with_eight_channels_per_head():
    _report("1x16x24, 8 channels per head", *_stats_case(1, 16, 24, [2], 905, CH=8))


# ----------------------------------------------------------------------------------------------------------- the composition
def _fold_inputs(B, H, W, seed):
    """partials of a statistics launch and the module's parameters (seeded)"""
    gram, s0, s1 = _stats_case(B, H, W, [3], seed, want=True)
    g = torch.Generator().manual_seed(seed + 9)
    r = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).cuda()
    params = (r(4).abs() + 0.5, r(4, 64, k=0.2), r(4, k=0.1), r(64, 4, k=0.5), r(64, k=0.1), r(64, 64, k=0.125), r(64, 128, k=0.09))
    ws, bs = PI._stencil_weights(seed + 2)
    return gram, s0, s1, params, ws, bs


def _fold_case(B, H, W, seed):
    from cdfo_amd import kernels as K
    gram, s0, s1, params, ws, bs = _fold_inputs(B, H, W, seed)
    n = gram.shape[1]
    stencil = K.pack_plane_chunk(ws, bs)
    full = K.align_fold(gram, n, s0, s1, n, H * W, *params)
    pc128, tables = K.align_fold_plane(gram, n, s0, s1, n, H * W, *params, stencil)
    torch.cuda.synchronize()
    return full, pc128, tables, stencil


@pytest.mark.parametrize("B,H,W", [(2, 8, 8), (5, 16, 24)])
def test_composition_behind_the_fold(B, H, W):
    full, pc128, tables, stencil = _fold_case(B, H, W, 40 + H)
    assert (pc128.Cin, pc128.Cout, pc128.CoutP, pc128.ks, pc128.w_bstride) == (128, 64, 64, 1, 128 * 64) and pc128.bias is None
    w192, w128 = full.w.view(B, 48, 64, 4), pc128.w.view(B, 32, 64, 4)          # [Cin/4][64][4]
    assert torch.equal(w128[:, :16], w192[:, :16]) and torch.equal(w128[:, 16:], w192[:, 32:])      # [M1 | Wb], bit for bit
    assert tuple(tables.shape) == (B, 64, 16) and tables.is_contiguous() and not tables[..., 10:].any()
    m2 = w192[:, 16:32].permute(0, 2, 1, 3).reshape(B, 64, 64)                   # M2[b][o][i]
    ref = m2.double() @ stencil.double()[:, :10]
    fp32 = torch.zeros(B, 64, 10, device="cuda")
    for i in range(64):                                                           # the fp32 product, i ascending
        fp32 = fp32 + m2[:, :, i, None] * stencil[i, None, None, :10]
    old = ((fp32.double() - ref).abs().max() / ref.abs().max()).item()
    new = ((tables[..., :10].double() - ref).abs().max() / ref.abs().max()).item()
    print(f"align_fold_plane {B}x{H}x{W}: tables rel {old:.2e} (fp32 product) -> {new:.2e}")
    assert new <= 4 * old, (old, new)


# ----------------------------------------------------------------------------------------------------------- determinism
def _dump(path):
    """the partials of one seeded statistics launch (several tiles per workgroup segment, two slots) and the fold's outputs -> path"""
    gram, s0, s1 = _stats_case(5, 16, 24, [1, 2], 4244, want=True)
    _, pc128, tables, _ = _fold_case(5, 16, 24, 4245)
    arrs = {k: v.cpu().numpy() for k, v in dict(gram=gram, s0=s0, s1=s1, w128=pc128.w, tables=tables).items()}
    if path:
        np.savez(path, **arrs)
    return arrs


def test_results_are_bitwise_reproducible(tmp_path):
    from conftest import clean_process_run
    first, second = _dump(None), _dump(None)
    assert all(first[k].tobytes() == second[k].tobytes() for k in first)
    path = str(tmp_path / "dump.npz")
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_gpu_prior_ufs as t; t._dump({path!r})"
    rc, so, se = clean_process_run([sys.executable, "-c", code], cwd=ROOT, timeout=120)
    assert rc == 0, se[-2000:]
    other = np.load(path)
    assert all(first[k].tobytes() == other[k].tobytes() for k in first)


# ----------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("B,H,W,seed", [(1, 24, 40, None), (1, 64, 64, 910)])
def test_forward_with_and_without_inline_ufs(B, H, W, seed):
    """model.inline_ufs (CDFO_INLINE_UFS) off and on, injected noise: L1_fea identical (the neighbour phase does not reach it), out
    within a tenth of the forward's parity bound; the first case is the 24x40 golden and is also held to the golden.  stem_conv
    launches per forward: 7 -> 1 (conv_first)."""
    from oracle.cvsr_v8_ref import make_inputs
    from cdfo_amd import kernels as K
    gold = None
    if seed is None:
        gold = np.load(os.path.join(ROOT, "tests", "golden", "cvsr_v8_b1_24x40.npz"))
        wseed, seed, layout = int(gold["wseed"]), int(gold["iseed"]), str(gold["layout"])
    else:
        wseed, layout = 21, "b1n"
    m = PI._model(wseed)
    inp = make_inputs(B, H, W, seed, layout)
    dev = {k: v.cuda() for k, v in inp.items() if k != "gumbel_u"}
    noise = [u.cuda() for u in inp["gumbel_u"]]
    res, calls = {}, {}
    real = K.stem_conv
    with torch.no_grad():
        for on in (False, True):
            m.inline_ufs = on
            n = [0]

            def counted(*a, **kw):
                n[0] += 1
                return real(*a, **kw)
            K.stem_conv = counted
            try:
                m.debug_taps = {}
                out, l1 = m(dev["x"], dev["mvs0"], dev["mvs1"], dev["pms"], dev["rms"], dev["ufs"], gumbel_uniform=noise)
            finally:
                K.stem_conv = real
            assert all(f"align_{i}" in m.debug_taps for i in (0, 1, 2, 4, 5, 6))      # debug_taps stays valid on both paths
            m.debug_taps = None
            res[on], calls[on] = (out.clone(), l1.clone()), n[0]
    torch.cuda.synchronize()
    d_out = (res[True][0] - res[False][0]).abs().max().item()
    print(f"inline_ufs off/on {B}x{H}x{W}: out {d_out:.2e}, stem_conv launches {calls[False]} -> {calls[True]}")
    assert (calls[False], calls[True]) == (7, 1)
    assert torch.equal(res[True][1], res[False][1])
    assert d_out <= 1e-4
    if gold is not None:
        assert (res[True][0].cpu() - torch.from_numpy(gold["out"])).abs().max().item() <= 1e-3


def test_chunk_sizes_1_and_4_agree_bit_for_bit_with_the_switch_on():
    """chunked inference with shared compensation (the frames= form of _align_group): a frame's result carries the same bits whether
    its window comes alone or with three others"""
    from cdfo_amd.streaming import StreamingSR
    from test_gpu_sequence import _model, _sequence
    from test_gpu_shared_compensation import _frame_noise
    T, H, W = 6, 16, 24
    _, model = _model(21)
    assert model.inline_ufs and model.align_stats and model.precision == "fp16x2"
    seq = _sequence(T, H, W, 6)
    u = [t.cuda() for t in _frame_noise(T, H, W, 800)]
    outs = {chunk: StreamingSR(model, *seq, frame_noise=u).run_chunked(chunk, share_compensation=True) for chunk in (1, 4)}
    assert len(outs[1]) == len(outs[4]) == T
    for a, b in zip(outs[1], outs[4]):
        assert torch.equal(a, b)
