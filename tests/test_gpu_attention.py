"""GPU parity of the LLongRangAttention kernels (rdab_prep in its three entry points, colconv9, seq_attn in its MFMA, PV1
and VALU forms, window form) against plain torch-cpu fp64 references on seeded inputs.  Inputs, references and tolerances
live in attn_cases.py; test_attention_cases_cpu.py shows that they catch defective kernels."""
import pytest
import torch

import attn_cases as AC

pytestmark = pytest.mark.gpu


def _ref(q, v, mode):
    B, H, W, C = q.shape
    if mode == 0:
        a = (q @ q.transpose(-1, -2)).softmax(-1)                      # [B,H,W,W]
        return a @ v
    if mode == 1:
        qt, vt = q.transpose(1, 2), v.transpose(1, 2)                  # [B,W,H,C]
        a = (qt @ qt.transpose(-1, -2)).softmax(-1)
        return (a @ vt).transpose(1, 2)
    qw = q.view(B, H // 8, 8, W // 8, 8, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 8, W // 8, 64, C)
    vw = v.view(B, H // 8, 8, W // 8, 8, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 8, W // 8, 64, C)
    o = (qw @ qw.transpose(-1, -2)).softmax(-1) @ vw
    return o.view(B, H // 8, W // 8, 8, 8, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)


@pytest.mark.parametrize("H,W", [(8, 8), (16, 40), (40, 136), (136, 72)])
@pytest.mark.parametrize("mode", [0, 1, 2, 10, 11, 12])
def test_seq_attn(H, W, mode):
    from cdfo_amd import kernels as K
    g = torch.Generator().manual_seed(H * 100 + W + mode)
    q = torch.randn(2, H, W, 64, generator=g) * 0.5
    v = torch.randn(2, H, W, 64, generator=g)
    ref = _ref(q, v, mode % 10)
    out = K.seq_attn(q.cuda(), v.cuda(), mode)
    torch.cuda.synchronize()
    err = (out.cpu() - ref).abs().max().item()
    assert err < 2e-5 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("C,H,W", [(192, 16, 24), (192, 9, 13), (64, 8, 8)])
def test_dwconv3x3(C, H, W):
    import torch.nn.functional as F
    from cdfo_amd import kernels as K
    g = torch.Generator().manual_seed(C + H + W)
    x = torch.randn(2, C, H, W, generator=g)
    w = torch.randn(C, 1, 3, 3, generator=g)
    ref = F.conv2d(x, w, padding=1, groups=C)
    out = K.dwconv3x3(x.permute(0, 2, 3, 1).contiguous().cuda(), w.cuda())
    torch.cuda.synchronize()
    assert (out.permute(0, 3, 1, 2).cpu() - ref).abs().max().item() < 1e-5


def _lt(err, bound, what):
    """test_qkv_dw_fused's error-against-bound assertions (tests/test_gpu_schedules.py records the ratios under a CU limit)"""
    assert err < bound, f"{what}: {err} (bound {bound})"


@pytest.mark.parametrize("B,H,W", [(2, 12, 30), (1, 17, 45), (3, 8, 64), (1, 5, 7), (2, 6, 121)])
def test_qkv_dw_fused(B, H, W):
    """LayerNorm -> 1x1 (64->192) -> depthwise 3x3 in one kernel vs the same chain in torch-cpu fp32."""
    import torch.nn.functional as F
    from cdfo_amd import kernels as K
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W)
    x = torch.randn(B, 64, H, W, generator=g) * 2 + 0.3
    gamma, beta = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    wq = torch.randn(192, 64, 1, 1, generator=g) / 8.0
    wd = torch.randn(192, 1, 3, 3, generator=g) / 3.0
    ln = F.layer_norm(x.permute(0, 2, 3, 1), (64,), gamma, beta, 1e-5).permute(0, 3, 1, 2)
    ref = F.conv2d(F.conv2d(ln, wq), wd, padding=1, groups=192)
    packed = K.pack_qkv_dw(wq.cuda(), gamma.cuda(), beta.cuda())
    out = K.qkv_dw(x.permute(0, 2, 3, 1).contiguous().cuda(), packed, wd.cuda().contiguous())
    torch.cuda.synchronize()
    err = (out.cpu().permute(0, 3, 1, 2) - ref).abs().max().item()
    _lt(err, 2e-5 * max(1.0, ref.abs().max().item()), "qkv_dw")
    # fused Gram mode: v only + the per-head sums sum_p q k^T, sum q^2, sum k^2 in cdfo_gram_partial's layout
    v, part, n = K.qkv_dw(x.permute(0, 2, 3, 1).contiguous().cuda(), packed, wd.cuda().contiguous(), gram=True)
    v2, part2, _ = K.qkv_dw(x.permute(0, 2, 3, 1).contiguous().cuda(), packed, wd.cuda().contiguous(), gram=True)
    assert torch.equal(part, part2) and torch.equal(v, v2)          # no atomics: bit-reproducible
    torch.cuda.synchronize()
    _lt((v.cpu().permute(0, 3, 1, 2) - ref[:, 128:]).abs().max().item(), 2e-5 * max(1.0, ref.abs().max().item()), "qkv_dw gram mode, v")
    q, k = ref[:, :64].double().reshape(B, 8, 8, H * W), ref[:, 64:128].double().reshape(B, 8, 8, H * W)
    want = torch.zeros(B, 64, 10, dtype=torch.float64)
    want[:, :, :8] = (q @ k.transpose(-1, -2)).reshape(B, 64, 8)
    want[:, :, 8] = (q * q).sum(-1).reshape(B, 64)
    want[:, :, 9] = (k * k).sum(-1).reshape(B, 64)
    got = part.cpu().double().sum(1).view(B, 64, 10)
    _lt((got - want).abs().max().item(), 1e-4 * max(1.0, want.abs().max().item()), "qkv_dw gram mode, slot sums")


# ----------------------------------------------------------------------------------- seq_attn at its edge shapes (attn_cases.py)
def _seq_attn_case(family, mode, B, H, W):
    """One seeded case against its fp64 reference: the three-pass rule, or the elementwise PV1 bound for modes 20 / 21 / 22."""
    from cdfo_amd import kernels as K
    q, v, ref, pav = AC.seq_case(family, mode % 10, B, H, W)
    out = K.seq_attn(q.cuda(), v.cuda(), mode)
    torch.cuda.synchronize()
    ratio = AC.seq_ratio(out.cpu(), ref, pav, mode, AC.seq_len(mode, H, W), v.abs().max().item())
    print(f"seq_attn mode {mode} {family} [{B},{H},{W}]: error / tolerance = {ratio:.4f}")
    assert ratio <= 1.0 if mode >= 20 else ratio < 1.0, ratio
    return out


@pytest.mark.parametrize("L", AC.SEQ_LENGTHS)
@pytest.mark.parametrize("mode", [0, 1, 20, 21])
def test_seq_attn_key_counts(mode, L):
    """1 / 8 keys in one tile; second stages of 1, 4, 5 keys (a half-wave fully masked); a masked sub-tile alone and as the
    second of an 8-wave stage; several workgroups per sequence with staging-only waves, waves past the end, a partly valid
    last query tile; a final stage of exactly 32 keys."""
    _seq_attn_case("spread", mode, 2, *AC.seq_shape(mode, L))


@pytest.mark.parametrize("L", [37, 272, 480])
@pytest.mark.parametrize("family", ["peaked", "offset"])
@pytest.mark.parametrize("mode", [0, 1, 20, 21])
def test_seq_attn_input_families(mode, family, L):
    _seq_attn_case(family, mode, 2, *AC.seq_shape(mode, L))


@pytest.mark.parametrize("L", [L for L in AC.SEQ_LENGTHS if L <= 168] + [272])
@pytest.mark.parametrize("mode", [10, 11])
def test_seq_attn_valu_key_counts(mode, L):
    _seq_attn_case("spread", mode, 2, *AC.seq_shape(mode, L))


@pytest.mark.parametrize("H,W", AC.WINDOW_SHAPES)
@pytest.mark.parametrize("family", ["spread", "peaked"])
@pytest.mark.parametrize("mode", [2, 12, 22])
def test_seq_attn_windows(mode, family, H, W):
    _seq_attn_case(family, mode, 2, H, W)


@pytest.mark.parametrize("mode,B,H,W", [(0, 1, 1, 272), (0, 1, 3, 272), (0, 2, 4, 272), (1, 1, 272, 3),
                                        (20, 1, 1, 272), (20, 1, 3, 272), (20, 2, 4, 272), (21, 1, 272, 3)])
def test_seq_attn_workgroup_remap(mode, B, H, W):
    """Three workgroups per sequence, grids of 3, 9 and 24: fewer than eight, no multiple of eight, a multiple of eight."""
    _seq_attn_case("spread", mode, B, H, W)


@pytest.mark.parametrize("mode,H,W", [(0, 3, 37), (1, 37, 3), (2, 8, 16), (0, 3, 272)])
def test_seq_attn_queries_on_fp16_ties(mode, H, W):
    """Queries whose product with log2 e is an exact fp16 tie (most elements here, 1 in 8192 of random inputs): the hi / lo
    split of the scaled query must add up whichever way the tie is rounded."""
    from cdfo_amd import kernels as K
    q, v, ref, pav, share = AC.tie_case(mode, 2, H, W)
    assert share > 0.5, share
    out = K.seq_attn(q.cuda(), v.cuda(), mode)
    torch.cuda.synchronize()
    ratio = AC.seq_ratio(out.cpu(), ref, pav, mode, AC.seq_len(mode, H, W), v.abs().max().item())
    print(f"seq_attn mode {mode} ties [2,{H},{W}]: error / tolerance = {ratio:.4f}")
    assert ratio < 1.0, ratio


_SENTINEL = 0x7FC12345       # a NaN's bit pattern: no kernel result looks like it


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("mode,H,W", [(0, 3, 37), (1, 37, 3), (2, 8, 16), (20, 3, 37), (21, 37, 3), (22, 8, 16), (0, 3, 272), (20, 3, 272)])
def test_seq_attn_strided_operands(mode, H, W, half):
    """As the model calls it: q and v the two halves of one 128-channel tensor, the result written into one half of another.
    Bit for bit the dense call's result, and the other half untouched."""
    from cdfo_amd import kernels as K
    q, v, _, _ = AC.seq_case("spread", mode % 10, 2, H, W)
    dense = _seq_attn_case("spread", mode, 2, H, W)
    x = torch.cat([q, v], -1).cuda()
    cat = torch.full((2, H, W, 128), _SENTINEL, dtype=torch.int32, device="cuda")
    mine, other = slice(64 * half, 64 * half + 64), slice(64 - 64 * half, 128 - 64 * half)
    ret = K.seq_attn(x[..., 0:64], x[..., 64:128], mode, out=cat.view(torch.float32)[..., mine])
    torch.cuda.synchronize()
    assert ret.data_ptr() == cat[..., mine].data_ptr()
    assert torch.equal(cat[..., mine].contiguous(), dense.view(torch.int32))
    assert (cat[..., other] == _SENTINEL).all()


@pytest.mark.parametrize("mode", [0, 1, 2, 20, 21, 22])
def test_seq_attn_is_deterministic(mode):
    """No atomics: two calls on the same inputs agree bit for bit."""
    from cdfo_amd import kernels as K
    for L in (272, 480):
        H, W = (L, 8) if mode % 10 == 2 else AC.seq_shape(mode, L)
        q, v, _, _ = AC.seq_case("spread", mode % 10, 2, H, W)
        qd, vd = q.cuda(), v.cuda()
        a, b = K.seq_attn(qd, vd, mode), K.seq_attn(qd, vd, mode)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------- rdab_prep
_RDAB_KEY, _RDAB_DRAW = 0x0123456789ABCDEF, 3


def _rdab_dev(B, H, W):
    xq, vmax, u, wW, bW = AC.rdab_inputs(B, H, W)
    return xq.cuda(), vmax.cuda(), u.cuda(), wW.cuda(), bW.cuda()


def _bit_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("B,H,W", AC.RDAB_SHAPES)
def test_rdab_prep(B, H, W):
    """Injected noise: the hard mask EXACTLY (recovered from the window query, no element excluded), the window query, and
    the 9-tap channel conv of the masked q and of v, against the fp64 reference.  Also the comparison that
    test_gumbel_mask_matches_the_oracle_and_the_inference_kernel's name promises: the training path's mask kernel decides
    every element as the inference kernel does."""
    from cdfo_amd import autograd as A
    from cdfo_amd import kernels as K
    xq, vmax, u, wW, bW = AC.rdab_inputs(B, H, W)
    assert AC.rdab_tie_distance(vmax, u) > 1e-5                      # the kernel decides in fp32
    d = _rdab_dev(B, H, W)
    sq, vrow, qwin = K.rdab_prep(*d)
    mask_train = A.gumbel_mask(d[1], d[2], B, H, W)
    torch.cuda.synchronize()
    AC.rdab_assert(sq.cpu(), vrow.cpu(), qwin.cpu(), AC.rdab_ref(xq, vmax, u, wW, bW))
    assert torch.equal(mask_train.cpu(), (qwin.cpu() == 0).float())
    again = K.rdab_prep(*d)
    assert _bit_equal(again, (sq, vrow, qwin))


@pytest.mark.parametrize("B,H,W", AC.RDAB_SHAPES)
def test_rdab_prep_rng(B, H, W):
    """Noise drawn in the kernel: the generator contract of numeric.h (Philox4x32-10, counter (p, b, c >> 2, draw), word c & 3,
    u = ((word >> 8) + 0.5) 2^-24) against a NumPy Philox; the drawn values, injected, reproduce all three outputs bit for bit;
    the key read from device memory gives the same bits; another draw or another key gives other noise."""
    from cdfo_amd import kernels as K
    xq, vmax, _, wW, bW = AC.rdab_inputs(B, H, W)
    want_u = AC.rdab_noise(B, H * W, _RDAB_KEY, _RDAB_DRAW).view(B, 64, H, W)
    assert AC.rdab_tie_distance(vmax, want_u) > 1e-5
    d = _rdab_dev(B, H, W)
    cap, cap_dev, cap_draw, cap_key = (torch.zeros(B, 64, H, W, device="cuda") for _ in range(4))
    drawn = K.rdab_prep_rng(d[0], d[1], _RDAB_KEY, _RDAB_DRAW, d[3], d[4], noise_out=cap)
    injected = K.rdab_prep(d[0], d[1], cap, d[3], d[4])
    key = torch.tensor([_RDAB_KEY], dtype=torch.int64, device="cuda")
    from_dev = K.rdab_prep_rng(d[0], d[1], key, _RDAB_DRAW, d[3], d[4], noise_out=cap_dev)
    K.rdab_prep_rng(d[0], d[1], _RDAB_KEY, _RDAB_DRAW + 1, d[3], d[4], noise_out=cap_draw)
    K.rdab_prep_rng(d[0], d[1], _RDAB_KEY + (1 << 32), _RDAB_DRAW, d[3], d[4], noise_out=cap_key)
    torch.cuda.synchronize()
    assert torch.equal(cap.cpu(), want_u)
    assert _bit_equal(drawn, injected) and _bit_equal(drawn, from_dev) and torch.equal(cap, cap_dev)
    assert not torch.equal(cap, cap_draw) and not torch.equal(cap, cap_key)
    AC.rdab_assert(drawn[0].cpu(), drawn[1].cpu(), drawn[2].cpu(), AC.rdab_ref(xq, vmax, want_u, wW, bW))


# -------------------------------------------------------------------------------------------------------------------- colconv9
def _colconv9_case(x_dev, x, ref):
    from cdfo_amd import kernels as K
    w, b = AC.col_weights()
    out = K.colconv9(x_dev, w.cuda(), b.cuda())
    torch.cuda.synchronize()
    want = ref(x, w, b)
    ratio = (out.cpu().double() - want).abs().max().item() / AC.tol_conv9(want)
    print(f"colconv9 {tuple(x.shape)}: error / tolerance = {ratio:.4f}")
    assert ratio < 1.0, ratio


@pytest.mark.parametrize("H", AC.COL_HEIGHTS)
def test_colconv9_heights(H):
    """Halo rows at both image edges, images shorter than the halo, rows on either side of the 34-row segment seams."""
    x = torch.randn(2, H, 5, 64, generator=torch.Generator().manual_seed(H))
    _colconv9_case(x.cuda(), x, AC.col_ref)


def test_colconv9_strided_input():
    big = torch.randn(2, 69, 5, 128, generator=torch.Generator().manual_seed(1))
    _colconv9_case(big.cuda()[..., 64:128], big[..., 64:128], AC.col_ref)


def test_colconv9_grid_stride():
    """More than the 8192 blocks one launch takes: the grid-stride loop runs (131080 columns x 16 channel groups / 256)."""
    x = torch.randn(1, 2, 131080, 64, generator=torch.Generator().manual_seed(2))
    _colconv9_case(x.cuda(), x, AC.col_ref_taps)
