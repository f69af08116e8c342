"""LLongRangAttention with input_conv inside the mask kernel (`kernels.rdab_prep_fused`) and with the V operands of the
single-pass attentions (modes 20-22) stored as fp16 (`kernels.seq_attn` with an fp16 v / out), against the launches they replace.

Nothing here has a tolerance.  The fused kernel runs the streaming 1x1 kernel's split-bf16 product instruction for instruction and
rdab_prep's sums in rdab_prep's order, so q, v, the mask and both channel convolutions carry the same bits; modes 20-22 round every
V once to fp16 while staging, so rounding at the producer instead is the same rounding.  Every comparison is `torch.equal`."""
import pytest
import torch

import attn_cases as AC

gpu = pytest.mark.gpu
FUSED_SHAPES = AC.RDAB_SHAPES + ((3, 16, 136),)        # the last: 51 tiles, so a persistent workgroup owns more than one where CUs are few
_KEY, _DRAW = 12345, 2


@pytest.fixture(scope="module")
def input_conv():
    """A seeded 64 -> 128 1x1 convolution with bias, packed, on the device."""
    from cdfo_amd import kernels as K
    g = torch.Generator().manual_seed(64128)
    wt = torch.randn(128, 64, 1, 1, generator=g) / 8.0
    b = torch.randn(128, generator=g) * 0.1
    return K.pack_conv(wt.cuda(), b.cuda())


def _operands(B, H, W):
    _, vmax, u, wW, bW = AC.rdab_inputs(B, H, W)
    g = torch.Generator().manual_seed((B * 131 + H) * 137 + W + 5)
    x = torch.randn(B, H, W, 64, generator=g)
    return x.cuda(), vmax.cuda(), u.cuda(), wW.cuda(), bW.cuda()


def _compare(new, old, xq_old):
    sq, vrow, qwin, vwin = new
    sq0, vrow0, qwin0 = old
    assert torch.equal((qwin == 0), (qwin0 == 0))                       # the mask, no element excluded
    assert torch.equal(sq, sq0) and torch.equal(qwin, qwin0)
    assert torch.equal(vrow, vrow0.to(vrow.dtype)) and torch.equal(vwin, xq_old[..., 64:].to(vwin.dtype))      # fp16: rounded once


@gpu
@pytest.mark.parametrize("v_f16", [True, False, (False, True)], ids=["f16", "f32", "vwin_f16"])
@pytest.mark.parametrize("B,H,W", FUSED_SHAPES)
def test_fused_kernel_equals_conv_then_prep_injected_noise(B, H, W, v_f16, input_conv):
    from cdfo_amd import kernels as K
    x, vmax, u, wW, bW = _operands(B, H, W)
    xq = K.conv(x, input_conv, prec=K.PREC_FP16X2)
    old = K.rdab_prep(xq, vmax, u, wW, bW)
    new = K.rdab_prep_fused(x, input_conv, vmax, u, wW, bW, v_f16=v_f16)
    torch.cuda.synchronize()
    _compare(new, old, xq)


@gpu
@pytest.mark.parametrize("B,H,W", FUSED_SHAPES)
def test_fused_kernel_equals_conv_then_prep_drawn_noise(B, H, W, input_conv):
    """The generator form, with the key as a launch argument and in device memory, and the drawn values captured."""
    from cdfo_amd import kernels as K
    x, vmax, _, wW, bW = _operands(B, H, W)
    xq = K.conv(x, input_conv, prec=K.PREC_FP16X2)
    cap0, cap1, cap2 = (torch.zeros(B, 64, H, W, device="cuda") for _ in range(3))
    key = torch.tensor([_KEY], dtype=torch.int64, device="cuda")
    old = K.rdab_prep_rng(xq, vmax, _KEY, _DRAW, wW, bW, noise_out=cap0)
    new = K.rdab_prep_fused(x, input_conv, vmax, ("rng", _KEY, _DRAW, cap1), wW, bW, v_f16=True)
    new_dev = K.rdab_prep_fused(x, input_conv, vmax, ("rng", key, _DRAW, cap2), wW, bW, v_f16=True)
    torch.cuda.synchronize()
    assert torch.equal(cap0.view(torch.int32), cap1.view(torch.int32)) and torch.equal(cap0.view(torch.int32), cap2.view(torch.int32))
    _compare(new, old, xq)
    _compare(new_dev, old, xq)


@gpu
@pytest.mark.parametrize("cus", [1, 4, 7])
def test_fused_kernel_with_many_tiles_per_workgroup(cus, input_conv):
    """3 x 16 x 136 = 51 tiles on 1, 4 and 7 workgroups: every workgroup walks several tiles through its ring (the scratch use of
    the stage just consumed, the request after next) and crosses image boundaries inside its range."""
    from cdfo_amd import kernels as K
    B, H, W = 3, 16, 136
    x, vmax, u, wW, bW = _operands(B, H, W)
    xq = K.conv(x, input_conv, prec=K.PREC_FP16X2)
    old = K.rdab_prep(xq, vmax, u, wW, bW)
    cap0, cap1 = (torch.zeros(B, 64, H, W, device="cuda") for _ in range(2))
    old_rng = K.rdab_prep_rng(xq, vmax, _KEY, _DRAW, wW, bW, noise_out=cap0)
    with K.cu_limit(cus):
        new = K.rdab_prep_fused(x, input_conv, vmax, u, wW, bW, v_f16=True)
        new_rng = K.rdab_prep_fused(x, input_conv, vmax, ("rng", _KEY, _DRAW, cap1), wW, bW, v_f16=False)
    torch.cuda.synchronize()
    _compare(new, old, xq)
    _compare(new_rng, old_rng, xq)
    assert torch.equal(cap0, cap1)


@gpu
def test_fused_kernel_on_a_slice_of_a_larger_batch(input_conv):
    """One neighbour's slice of the group's tensors, as `_rdab` calls it: outputs outside the slice stay untouched."""
    from cdfo_amd import kernels as K
    B, H, W = 2, 16, 24
    x, vmax, u, wW, bW = _operands(2 * B, H, W)
    sl = slice(B, 2 * B)
    outs = [torch.full((2 * B, H, W, 64), 7.0, dtype=dt, device="cuda") for dt in (torch.float32, torch.float16, torch.float32, torch.float16)]
    K.rdab_prep_fused(x[sl], input_conv, vmax[sl], u[sl].contiguous(), wW, bW, v_f16=True, outs=tuple(t[sl] for t in outs))
    xq = K.conv(x[sl], input_conv, prec=K.PREC_FP16X2)
    old = K.rdab_prep(xq, vmax[sl], u[sl].contiguous(), wW, bW)
    torch.cuda.synchronize()
    _compare(tuple(t[sl] for t in outs), old, xq)
    assert all(bool((t[:B] == 7.0).all()) for t in outs)


# --------------------------------------------------------------------------------------------------------------- fp16 V
def _seq(family, mode, H, W, B=2):
    q, v, _, _ = AC.seq_case(family, mode % 10, B, H, W)
    return q.cuda(), v.cuda()


@gpu
@pytest.mark.parametrize("family", ["spread", "offset"])
@pytest.mark.parametrize("L", [1, 33, 136, 300])
@pytest.mark.parametrize("mode", [20, 21])
def test_fp16_v_gives_the_bits_of_fp32_v_rows_and_columns(mode, L, family):
    from cdfo_amd import kernels as K
    q, v = _seq(family, mode, *AC.seq_shape(mode, L))
    want = K.seq_attn(q, v, mode)
    got = K.seq_attn(q, v.half(), mode)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and torch.equal(got, want)
    if mode == 20:
        h0 = K.seq_attn(q, v, mode, out_dtype=torch.float16)
        h1 = K.seq_attn(q, v.half(), mode, out=torch.empty(q.shape, dtype=torch.float16, device="cuda"))
        torch.cuda.synchronize()
        assert h0.dtype == torch.float16 and torch.equal(h0, want.half()) and torch.equal(h1, want.half())


@gpu
@pytest.mark.parametrize("family", ["spread", "offset"])
@pytest.mark.parametrize("H,W", [(8, 8), (24, 8), (16, 40)])
def test_fp16_v_gives_the_bits_of_fp32_v_windows(H, W, family):
    from cdfo_amd import kernels as K
    q, v = _seq(family, 22, H, W)
    want = K.seq_attn(q, v, 22)
    got = K.seq_attn(q, v.half(), 22)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


@gpu
def test_fp16_v_as_a_channel_slice():
    """v and out as 64-channel slices of wider tensors (pitches counted in halves / floats)."""
    from cdfo_amd import kernels as K
    q, v = _seq("spread", 21, 40, 8)
    wide = torch.zeros(*v.shape[:3], 128, dtype=torch.float16, device="cuda")
    wide[..., 64:] = v.half()
    cat = torch.zeros(*v.shape[:3], 128, device="cuda")
    K.seq_attn(q, wide[..., 64:], 21, out=cat[..., 0:64])
    want = K.seq_attn(q, v, 21)
    torch.cuda.synchronize()
    assert torch.equal(cat[..., 0:64], want) and bool((cat[..., 64:] == 0).all())


# --------------------------------------------------------------------------------------------------------------- module
@gpu
@pytest.mark.parametrize("precision", ["fp16x2", "bf16x3"])
def test_rdab_module_with_the_switch_on_and_off(precision):
    """`_rdab` on a group of two neighbours, B = 2, 16x24, injected noise: model.rdab_fused (CDFO_RDAB_FUSED) on against off.
    fp16x2 takes the fp16 V operands as well, bf16x3 the fused kernel with fp32 V and the three-pass attentions."""
    from arch.SIDECVSR_our import CVSR_V8
    from oracle.cvsr_v8_ref import make_state_dict
    m = CVSR_V8()
    m.load_state_dict(make_state_dict(21), strict=True)
    m = m.cuda().eval()
    m.precision = precision
    G, B, H, W = 2, 2, 16, 24
    g = torch.Generator().manual_seed(1624)
    x = torch.randn(G * B, H, W, 64, generator=g).cuda()
    du0 = torch.rand(G * B, H // 2 + 1, W // 2 + 1, 256, generator=g).cuda()
    noises = [AC.rdab_inputs(B, H, W, seed=s)[2].cuda() for s in range(G)]
    res = {}
    with torch.no_grad():
        for on in (False, True):
            m.rdab_fused = on
            res[on] = m._rdab(m._weights(), du0, x, noises).clone()
    torch.cuda.synchronize()
    assert torch.equal(res[True], res[False])


# --------------------------------------------------------------------------------------------------------------- wrapper (no GPU)
@pytest.mark.parametrize("mode", [0, 1, 2, 10, 11, 12, 3])
def test_fp16_operands_outside_the_single_pass_modes_raise(mode):
    from cdfo_amd import kernels as K
    q = torch.zeros(1, 8, 8, 64)
    with pytest.raises(ValueError, match="fp16"):
        K.seq_attn(q, q.half(), mode)
    with pytest.raises(ValueError, match="fp16"):
        K.seq_attn(q, q, mode, out_dtype=torch.float16)


@pytest.mark.parametrize("mode", [21, 22])
def test_an_fp16_output_is_the_row_form_only(mode):
    from cdfo_amd import kernels as K
    q = torch.zeros(1, 8, 8, 64)
    with pytest.raises(ValueError, match="fp16"):
        K.seq_attn(q, q.half(), mode, out=torch.zeros(1, 8, 8, 64, dtype=torch.float16))
