"""`model.stack_inplace` (CDFO_STACK_INPLACE): the neighbour phase reads the feature stack where the extractor wrote it.  Its seven
readers take an image map (`kernels.image_map`, csrc/image_map.h) where they took a dense tensor [M,H,W,64]:

    1  rdab_prep_fused            x                      (plane form)
    2  conv, streaming 1x1        res1                   (RDAB.fuse, plane form)
    3  conv, streaming 1x1        second source          (the folded alignment convolution: per-image weights, plane, channel sums)
    4  conv, tiled 1x1            the fourth of seven sources (tsa_fusion: 448 channels, beyond the streaming kernel's LDS)
    5  align_stats                q                      (with x1 in memory and with the plane)
    6  conv3x3_ws_res             res2
    7  conv, tiled 3x3            source 0               (conv_expand_fea_r, split-fp16 and split-bf16)

Only addresses change, so every check here is `torch.equal`: each kernel runs once on a mapped operand taken from a clip-major stack
[B,7,H,W,ld] whose other slots hold 100.0 (a read across an image's end would show at that size), and once on the materialised dense
copy of the same images.  Shapes: half a tile (8x8); a wave's 32 pixels spanning two rows (16x24); every pixel on a border (2x64,
64x2); 7.5 tiles (24x40); B in {1, 2, 3} clips and G in {1, 3} frames per group, so that image m needs both strides; a pixel pitch of
80 floats; 5x16x24 on 1, 4 and 7 CUs for the persistent kernels (several tiles per ring, segments crossing images).  The three shapes
of the map: a group's frames (Bi = B, s_b = 7 P ld, s_g = P ld), one frame of every clip (s_g = 0), the centre once per neighbour
(M = G B, s_g = 0).  Then the whole forward with the switch off and on, and chunked inference at chunk sizes 1 and 4.
"""
import os

import numpy as np
import pytest
import torch

import attn_cases as AC
import test_gpu_prior_inline as PI

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B clips, G frames of a group, H, W, pixel pitch)
CASES = [(1, 1, 8, 8, 64), (2, 3, 8, 8, 64), (3, 3, 16, 24, 64), (1, 3, 2, 64, 64), (2, 1, 64, 2, 64), (1, 3, 24, 40, 64), (2, 3, 16, 24, 80)]
IDS = [f"B{b}G{g}_{h}x{w}_ld{ld}" for b, g, h, w, ld in CASES]


def _feature_stack(B, H, W, ld, seed, frames):
    """clip-major [B,7,H,W,ld], every float 100.0 but the 64 channels of the named frames"""
    g = torch.Generator().manual_seed(seed)
    st = torch.full((B, 7, H, W, ld), 100.0)
    for i in frames:
        st[:, i, :, :, :64] = torch.randn(B, H, W, 64, generator=g)
    return st.cuda()


def _group(st, i0, G):
    """frames i0 .. i0 + G - 1 of every clip, neighbour major -> (map, dense copy)"""
    from cdfo_amd import kernels as K
    B, _, H, W, ld = st.shape
    m = K.image_map(st[0, i0, :, :, :64], G * B, B, 7 * H * W * ld, H * W * ld)
    dense = torch.stack([st[b, i0 + g, :, :, :64] for g in range(G) for b in range(B)]).contiguous()
    assert torch.equal(m.dense(), dense)
    return m, dense


def _centre(st, i, G):
    """frame i of every clip once per neighbour -> (map, dense copy)"""
    from cdfo_amd import kernels as K
    B, _, H, W, ld = st.shape
    m = K.image_map(st[0, i, :, :, :64], G * B, B, 7 * H * W * ld, 0)
    dense = st[:, i, :, :, :64].repeat(G, 1, 1, 1).contiguous()
    assert torch.equal(m.dense(), dense)
    return m, dense


def _same(a, b):
    a, b = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    torch.cuda.synchronize()
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, torch.Tensor):
            assert x.shape == y.shape and torch.equal(x, y)
        else:
            assert x == y


# ----------------------------------------------------------------------------------------------------------- 1: the mask kernel
def _mask_case(B, G, H, W, ld, seed):
    """one launch per neighbour, its B images one clip stride apart (what _rdab launches), x + the plane"""
    from cdfo_amd import kernels as K
    g = torch.Generator().manual_seed(64128)
    wt, bt = (torch.randn(128, 64, 1, 1, generator=g) / 8.0).cuda(), (torch.randn(128, generator=g) * 0.1).cuda()
    pc = K.pack_conv(wt, bt)
    st = _feature_stack(B, H, W, ld, seed, range(2, 2 + G))
    m, dense = _group(st, 2, G)
    planes = PI._stack(B, H, W, seed + 1, list(range(2, 2 + G)))
    ws, bs = PI._stencil_weights(seed + 2)
    table = K.pack_plane_chunk(*K.compose_stem_1x1(ws, bs, wt, torch.zeros_like(bt)))
    _, vmax, u, wW, bW = (t.cuda() for t in AC.rdab_inputs(G * B, H, W))
    for n in range(G):
        sl = slice(n * B, (n + 1) * B)
        plane = (planes[:, 0, 2 + n], B, 7 * H * W, 0, table)
        for f16 in (False, True):
            new = K.rdab_prep_fused(m.sub(n * B, B), pc, vmax[sl], u[sl].contiguous(), wW, bW, v_f16=f16, plane=plane)
            old = K.rdab_prep_fused(dense[sl], pc, vmax[sl], u[sl].contiguous(), wW, bW, v_f16=f16, plane=plane)
            _same(new, old)


@pytest.mark.parametrize("B,G,H,W,ld", [c for c in CASES if c[2] * c[3] % 64 == 0], ids=[i for c, i in zip(CASES, IDS) if c[2] * c[3] % 64 == 0])
def test_mask_kernel_reads_x_through_the_map(B, G, H, W, ld):
    _mask_case(B, G, H, W, ld, 100 + H)


# ----------------------------------------------------------------------------------------------------------- 2-4: the 1x1 kernels
def _fuse_case(B, G, H, W, ld, seed):
    """RDAB.fuse: fuse(cat) + (fea + stencil(plane)) with fea mapped; and the same product without the plane"""
    from cdfo_amd import kernels as K
    st = _feature_stack(B, H, W, ld, seed, range(4, 4 + G))
    m, dense = _group(st, 4, G)
    M = G * B
    g = torch.Generator().manual_seed(seed + 1)
    cat = torch.randn(M, H, W, 128, generator=g).cuda()
    wf, bf = (torch.randn(64, 128, 1, 1, generator=g) / 11).cuda(), (torch.randn(64, generator=g) * 0.1).cuda()
    pc = K.pack_conv(wf, bf)
    planes = PI._stack(B, H, W, seed + 3, list(range(4, 4 + G)))
    ws, bs = PI._stencil_weights(seed + 2)
    plane = (planes[:, 0, 4], B, 7 * H * W, H * W if G > 1 else 0, K.pack_plane_chunk(ws, bs))
    for prec in (K.PREC_FP16X2, K.PREC_BF16X3):
        _same(K.conv(cat, pc, res1=m, prec=prec, plane=plane), K.conv(cat, pc, res1=dense, prec=prec, plane=plane))
        _same(K.conv(cat, pc, res1=m, prec=prec), K.conv(cat, pc, res1=dense, prec=prec))
        _same(K.conv(cat, pc, res1=cat[..., :64], res2=m, act=K.ACT_LRELU, prec=prec),
              K.conv(cat, pc, res1=cat[..., :64], res2=dense, act=K.ACT_LRELU, prec=prec))


def _folded_case(B, G, H, W, ld, seed):
    """the folded alignment convolution: relu(W_b . [x0; stencil; xc]) with per-image weights and channel sums, xc = the centre once
    per neighbour; and its form with pred in memory (three sources)"""
    from cdfo_amd import kernels as K
    st = _feature_stack(B, H, W, ld, seed, [3])
    m, dense = _centre(st, 3, G)
    M = G * B
    g = torch.Generator().manual_seed(seed + 1)
    x0, pred = torch.randn(M, H, W, 64, generator=g).cuda(), torch.randn(M, H, W, 64, generator=g).cuda()
    wb = (torch.randn(M, 64, 192, generator=g) / 13).cuda()
    bias = (torch.randn(64, generator=g) * 0.1).cuda()
    ws, bs = PI._stencil_weights(seed + 2)
    pk = lambda w: torch.cat([K.pack_conv(w[i].reshape(64, -1, 1, 1).contiguous(), None).w for i in range(M)])
    pc192 = K.PackedConv(pk(wb), bias, 64, 192, 1, 64, w_bstride=192 * 64)
    pc128 = K.PackedConv(pk(torch.cat([wb[:, :, :64], wb[:, :, 128:]], 2)), bias, 64, 128, 1, 64, w_bstride=128 * 64)
    zero = torch.zeros(64, device="cuda")
    tables = torch.stack([K.pack_plane_chunk(*K.compose_stem_1x1(ws, bs, wb[i, :, 64:128].reshape(64, 64, 1, 1), zero))
                          for i in range(M)]).contiguous()
    planes = PI._stack(B, H, W, seed + 3, list(range(0, G)))
    plane = (planes[:, 0, 0], B, 7 * H * W, H * W if G > 1 else 0, tables, 64 * 16)
    kw = dict(act=K.ACT_RELU, prec=K.PREC_FP16X2, chan_sum_out=True)
    _same(K.conv([x0, m], pc128, plane=plane, **kw), K.conv([x0, dense], pc128, plane=plane, **kw))
    _same(K.conv([x0, pred, m], pc192, **kw), K.conv([x0, pred, dense], pc192, **kw))


def _tsa_case(B, H, W, ld, seed):
    """tsa_fusion: seven 64-channel sources, the fourth the centre frame of every clip read from the stack (the tiled 1x1 kernel)"""
    from cdfo_amd import kernels as K
    st = _feature_stack(B, H, W, ld, seed, [3])
    m, dense = _centre(st, 3, 1)
    g = torch.Generator().manual_seed(seed + 1)
    al = [torch.randn(B, H, W, 64, generator=g).cuda() for _ in range(6)]
    wt, bt = (torch.randn(64, 448, 1, 1, generator=g) / 21).cuda(), (torch.randn(64, generator=g) * 0.1).cuda()
    pc = K.pack_conv(wt, bt)
    assert not K.conv1x1_map_ok(448, res=True) and K.conv_map_ok(pc, K.PREC_FP16X2)      # beyond the streaming kernel: the tiled one
    for prec in (K.PREC_FP16X2, K.PREC_BF16X3):
        _same(K.conv([*al[:3], m, *al[3:]], pc, act=K.ACT_LRELU, prec=prec), K.conv([*al[:3], dense, *al[3:]], pc, act=K.ACT_LRELU, prec=prec))


@pytest.mark.parametrize("B,G,H,W,ld", CASES, ids=IDS)
def test_one_by_one_kernels_read_their_operands_through_the_map(B, G, H, W, ld):
    _fuse_case(B, G, H, W, ld, 200 + H)
    _folded_case(B, G, H, W, ld, 300 + H)
    _tsa_case(B, H, W, ld, 400 + H)


# ----------------------------------------------------------------------------------------------------------- 5: the statistics
def _stats_case(B, G, H, W, ld, seed):
    from cdfo_amd import kernels as K
    st = _feature_stack(B, H, W, ld, seed, [3])
    m, dense = _centre(st, 3, G)
    M = G * B
    g = torch.Generator().manual_seed(seed + 1)
    x0 = (torch.randn(M, H, W, 64, generator=g) * torch.linspace(0.5, 2.0, 64) + 0.25).cuda()
    x1 = torch.randn(M, H, W, 64, generator=g).cuda()
    wt, bt = (torch.randn(64, 128, 1, 1, generator=g) / 128 ** 0.5).cuda(), (torch.randn(64, generator=g) * 0.1).cuda()
    ws, bs = PI._stencil_weights(seed + 2)
    pc = K.pack_conv(wt, bt)
    table = K.pack_plane_chunk(*K.compose_stem_1x1(ws, bs, wt[:, 64:], torch.zeros_like(bt)))
    planes = PI._stack(B, H, W, seed + 3, list(range(4, 4 + G)))
    plane = (planes[:, 0, 4], B, 7 * H * W, H * W if G > 1 else 0, table, K.pack_plane_chunk(ws, bs))
    for CH in (16, 8):
        _same(K.align_stats(x0, None, m, pc, K.ACT_RELU, CH, plane=plane), K.align_stats(x0, None, dense, pc, K.ACT_RELU, CH, plane=plane))
        _same(K.align_stats(x0, x1, m, pc, K.ACT_RELU, CH), K.align_stats(x0, x1, dense, pc, K.ACT_RELU, CH))


@pytest.mark.parametrize("B,G,H,W,ld", CASES, ids=IDS)
def test_statistics_kernel_reads_q_through_the_map(B, G, H, W, ld):
    _stats_case(B, G, H, W, ld, 500 + H)


# ----------------------------------------------------------------------------------------------------------- 6, 7: the 3x3 kernels
def _ws_res_case(B, G, H, W, ld, seed):
    from cdfo_amd import kernels as K
    st = _feature_stack(B, H, W, ld, seed, [3])
    m, dense = _centre(st, 3, G)
    M = G * B
    g = torch.Generator().manual_seed(seed + 1)
    x, o = torch.randn(M, H, W, 64, generator=g).cuda(), torch.randn(M, H, W, 64, generator=g).cuda()
    pc = K.pack_conv((torch.randn(64, 64, 3, 3, generator=g) / 24).cuda(), (torch.randn(64, generator=g) * 0.1).cuda())
    assert pc.wh is not None and K.ws_res_map_ok(M, H, W)
    x16 = K.to_cp16(x)
    c_new, c_old = torch.empty_like(x16), torch.empty_like(x16)
    _same((K.conv3x3_ws_res(x16, pc, res1=o, res2=m, out2_cp16=c_new), c_new), (K.conv3x3_ws_res(x16, pc, res1=o, res2=dense, out2_cp16=c_old), c_old))


def _fea_r_case(B, G, H, W, ld, seed):
    """conv_expand_fea_r([fea, x_n]): source 0 the group's frames read from the stack"""
    from cdfo_amd import kernels as K
    st = _feature_stack(B, H, W, ld, seed, range(0, G))
    m, dense = _group(st, 0, G)
    M = G * B
    g = torch.Generator().manual_seed(seed + 1)
    x_n = torch.randn(M, H, W, 64, generator=g).cuda()
    pc = K.pack_conv((torch.randn(64, 128, 3, 3, generator=g) / 34).cuda(), (torch.randn(64, generator=g) * 0.1).cuda())
    for prec in (K.PREC_FP16X2, K.PREC_BF16X3):
        assert K.conv_map_ok(pc, prec, pad=1)
        _same(K.conv([m, x_n], pc, pad=1, prec=prec), K.conv([dense, x_n], pc, pad=1, prec=prec))


@pytest.mark.parametrize("B,G,H,W,ld", CASES, ids=IDS)
def test_three_by_three_kernels_read_their_operands_through_the_map(B, G, H, W, ld):
    if H % 2 == 0:      # (the weights-stationary kernels walk pairs of rows)
        _ws_res_case(B, G, H, W, ld, 600 + H)
    _fea_r_case(B, G, H, W, ld, 700 + H)


# ----------------------------------------------------------------------------------------------------------- a limited CU share
@pytest.mark.parametrize("cus", [1, 4, 7])
def test_persistent_kernels_with_many_tiles_per_workgroup(cus):
    """5 clips x 16 x 24 = 15 tiles per frame on 1, 4 and 7 workgroups: several tiles per ring, segments crossing images"""
    from cdfo_amd import kernels as K
    with K.cu_limit(cus):
        _mask_case(5, 1, 16, 24, 64, 810)
        _fuse_case(5, 1, 16, 24, 64, 820)
        _folded_case(5, 1, 16, 24, 64, 830)
        _stats_case(5, 1, 16, 24, 64, 840)
        _fuse_case(5, 3, 16, 24, 80, 850)
        _stats_case(5, 3, 16, 24, 80, 860)


def test_operands_a_kernel_cannot_map_are_refused():
    from cdfo_amd import kernels as K
    st = _feature_stack(2, 8, 8, 64, 5, [3])
    m, dense = _centre(st, 3, 1)
    pc = K.pack_conv(torch.randn(64, 64, 1, 1).cuda(), None)
    with pytest.raises(ValueError):
        K.conv(m, pc, prec=K.PREC_F32)                        # the exact-fp32 kernels take no map
    with pytest.raises(ValueError):
        K.rdab_prep_fused(m, K.pack_conv(torch.randn(128, 64, 1, 1).cuda(), None), *[t.cuda() for t in AC.rdab_inputs(2, 8, 8)][1:])
    with pytest.raises(ValueError):
        K.image_map(st[0, 3, :, :, :64], 2, 2, 7 * 64 * 64 + 2, 0)      # a stride that leaves 16-byte alignment
    with pytest.raises(ValueError):
        K.image_map(st[0, 3, :, :, :64], 3, 3, 7 * 64 * 64, 0)          # a third clip: beyond the storage


# ----------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("B,H,W,seed", [(2, 24, 40, None), (1, 64, 64, 910)])
def test_forward_with_and_without_the_stack_in_place(B, H, W, seed):
    """model.stack_inplace (CDFO_STACK_INPLACE) off and on, injected noise: out and L1_fea bit for bit; the first case has the 24x40
    golden's weights and inputs seed at two clips.  With the switch on no frame-major copy is made and nothing is repeated."""
    from oracle.cvsr_v8_ref import make_inputs
    from cdfo_amd import kernels as K
    if seed is None:
        gold = np.load(os.path.join(ROOT, "tests", "golden", "cvsr_v8_b1_24x40.npz"))
        wseed, seed, layout = int(gold["wseed"]), int(gold["iseed"]), str(gold["layout"])
    else:
        wseed, layout = 21, "b1n"
    m = PI._model(wseed)
    inp = make_inputs(B, H, W, seed, layout)
    dev = {k: v.cuda() for k, v in inp.items() if k != "gumbel_u"}
    noise = [u.cuda() for u in inp["gumbel_u"]]
    res, swaps, maps = {}, {}, {}
    real_swap, real_map = K.swap_outer, K.image_map
    with torch.no_grad():
        for on in (False, True):
            m.stack_inplace = on
            n = [0, 0]

            def swap(*a, **kw):
                n[0] += 1
                return real_swap(*a, **kw)

            def mapped(*a, **kw):
                n[1] += 1
                return real_map(*a, **kw)
            K.swap_outer, K.image_map = swap, mapped
            try:
                m.debug_taps = {}
                out, l1 = m(dev["x"], dev["mvs0"], dev["mvs1"], dev["pms"], dev["rms"], dev["ufs"], gumbel_uniform=noise)
            finally:
                K.swap_outer, K.image_map = real_swap, real_map
            assert all(f"align_{i}" in m.debug_taps and f"rdab_{i}" in m.debug_taps for i in (0, 1, 2, 4, 5, 6))
            m.debug_taps = None
            res[on], swaps[on], maps[on] = (out.clone(), l1.clone()), n[0], n[1]
    torch.cuda.synchronize()
    print(f"stack_inplace off/on {B}x{H}x{W}: swap_outer launches {swaps[False]} -> {swaps[True]}, image maps {maps[False]} -> {maps[True]}")
    assert swaps[True] == 0 and maps[False] == 0 and maps[True] > 0 and swaps[False] == (1 if B > 1 else 0)
    assert torch.equal(res[True][0], res[False][0])
    assert torch.equal(res[True][1], res[False][1])


@pytest.mark.parametrize("share", [False, True])
def test_chunk_sizes_1_and_4_agree_bit_for_bit_with_the_switch_on(share):
    """chunked inference (forward_windows: the frame-major window stack read through maps with its own strides; with shared
    compensation the centres once per neighbour): a frame's result carries the same bits whether its window comes alone or with three
    others, and the bits of the path without the switch"""
    from cdfo_amd.streaming import StreamingSR
    from test_gpu_sequence import _model, _sequence
    from test_gpu_shared_compensation import _frame_noise, _tied
    T, H, W = 6, 16, 24
    _, model = _model(21)
    assert model.stack_inplace and model.precision == "fp16x2"
    seq = _sequence(T, H, W, 6)
    u = [t.cuda() for t in _frame_noise(T, H, W, 800)]
    # injected noise in both modes: one draw per frame (shared), the same draws per (window, slot) (unshared)
    kw = dict(frame_noise=u) if share else dict(gumbel_uniform=_tied(u, T))
    outs = {chunk: StreamingSR(model, *seq, **kw).run_chunked(chunk, share_compensation=share) for chunk in (1, 4)}
    model.stack_inplace = False
    try:
        off = StreamingSR(model, *seq, **kw).run_chunked(4, share_compensation=share)
    finally:
        model.stack_inplace = True
    assert len(outs[1]) == len(outs[4]) == len(off) == T
    for a, b, c in zip(outs[1], outs[4], off):
        assert torch.equal(a, b) and torch.equal(b, c)
