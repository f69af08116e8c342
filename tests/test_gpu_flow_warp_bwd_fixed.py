"""`cdfo_flow_warp_bwd_fixed` (csrc/train_ops.hip), the flow warp's adjoint as fixed-point integer sums, through the autograd
Function that uses it: against torch's fp64 autograd of the oracle's `flow_warp`; equal bits from call to call where many sources
fall on one destination (the case in which fp32 atomics change their low bits from run to run); a non-finite gradient still
propagates; without the switch the path is the fp32-atomic one as before; and with it one `CVSR_V8` training step gives equal parameter gradients twice."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def fixed_scatter(monkeypatch):
    """`autograd.FLOW_WARP_FIXED`, which `train.fit` sets for a run with the LPIPS term"""
    from cdfo_amd import autograd as A
    monkeypatch.setattr(A, "FLOW_WARP_FIXED", True)


def _case(B, H, W, Cc, seed, collide):
    """(gradient at the output [B,H,W,Cc], flow [B,2,H,W]); ``collide``: every source samples the neighbourhood of ONE pixel, so
    that four destinations take H W contributions each."""
    rs = np.random.RandomState(seed)
    g = (rs.randn(B, H, W, Cc) * np.exp(rs.uniform(-6, 6, (B, H, W, 1)))).astype(np.float32)      # magnitudes over five decades
    if collide:
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        mv = np.stack([W // 2 + 0.3 - xx, H // 2 + 0.6 - yy]).astype(np.float32)[None].repeat(B, 0)
    else:
        mv = (rs.randn(B, 2, H, W) * 2.5).astype(np.float32)
    return torch.from_numpy(g), torch.from_numpy(np.ascontiguousarray(mv))


def _backward(g, mv):
    from cdfo_amd import autograd as A
    B, H, W, Cc = g.shape
    x = torch.zeros((B, H, W, Cc), device="cuda", requires_grad=True)
    A.flow_warp(x, mv.cuda(), 2 * H * W).backward(g.cuda())
    return x.grad.cpu()


def _backward_atomic(g, mv):
    """cdfo_flow_warp_bwd, the fp32-atomic scatter, on the same operands"""
    from cdfo_amd import _lib
    B, H, W, Cc = g.shape
    gd, md, dx = g.cuda(), mv.cuda(), torch.zeros((B, H, W, Cc), device="cuda")
    rc = _lib.lib().cdfo_flow_warp_bwd(C.c_void_p(gd.data_ptr()), Cc, C.c_void_p(md.data_ptr()), C.c_longlong(2 * H * W), B, H, W, Cc,
                                       C.c_void_p(dx.data_ptr()), Cc, None)
    assert rc == 0
    torch.cuda.synchronize()
    return dx.cpu()


@pytest.mark.parametrize("B,H,W,Cc,collide", [(2, 12, 16, 64, False), (1, 5, 7, 4, False), (2, 9, 11, 16, True), (1, 33, 47, 8, True)])
def test_matches_the_oracle_and_the_atomic_form_and_repeats_bit_for_bit(B, H, W, Cc, collide):
    """Against torch's fp64 autograd of the oracle's flow_warp: 2e-4 of max(1, largest |gradient|), the bound
    tests/test_gpu_autograd_ops.py holds this operator to (the sample coordinates are fp32 on the device).  Against the fp32-atomic
    form, which adds the SAME fp32 contributions v: recursive fp32 summation of n terms is within (n - 1) 2^-24 sum |v| of their
    exact sum, the fixed-point sum within n / 2 units (2^-47 of the largest |g| or less here) and one rounding, 2^-24 |sum|; a
    destination takes at most n = H W terms, and sum |v| is the same backward of |g|.  So elementwise
    |fixed - atomic| <= H W 2^-24 sum |v| + H W 2^-47 max |g|."""
    from oracle.cvsr_v8_ref import flow_warp
    g, mv = _case(B, H, W, Cc, 7 * H + W + Cc, collide)
    x = torch.zeros((B, Cc, H, W), dtype=torch.float64, requires_grad=True)
    flow_warp(x, mv.double().permute(0, 2, 3, 1)).backward(g.double().permute(0, 3, 1, 2))
    want = x.grad.permute(0, 2, 3, 1)
    got = _backward(g, mv)
    err = float((got.double() - want).abs().max())
    print(f"{B}x{H}x{W}x{Cc} collide={collide}: {err:.3g} against the oracle, largest |gradient| {float(want.abs().max()):.3g}")
    assert bool(torch.isfinite(got).all()) and err <= 2e-4 * max(1.0, float(want.abs().max()))
    n = H * W
    bound = n * 2.0 ** -24 * _backward(g.abs(), mv).double() + n * 2.0 ** -47 * float(g.abs().max())
    gap = (got.double() - _backward_atomic(g, mv).double()).abs()
    print(f"  against the fp32 atomics: worst gap {float(gap.max()):.3g}, worst share of its bound {float((gap / bound.clamp_min(1e-300)).max()):.3g}")
    assert bool((gap <= bound).all())
    for _ in range(3):
        assert torch.equal(_backward(g, mv).view(torch.int32), got.view(torch.int32))


def test_switch_off_is_the_atomic_form(monkeypatch):
    """The default path against the entry point it always called.  Two fp32 summations of the same n <= H W = 35 terms in different
    orders are each within (n - 1) 2^-24 sum |v| of the exact sum, so within 70 x 2^-24 sum |v| of each other."""
    from cdfo_amd import autograd as A
    monkeypatch.setattr(A, "FLOW_WARP_FIXED", False)
    g, mv = _case(1, 5, 7, 4, 5, False)
    got, want = _backward(g, mv), _backward_atomic(g, mv)
    assert float((got - want).abs().max()) <= 70 * 2.0 ** -24 * float(_backward(g.abs(), mv).max())


def test_non_finite_gradient_propagates():
    g, mv = _case(1, 6, 8, 4, 3, False)
    g[0, 2, 3, 1] = float("inf")
    g[0, 4, 4, 2] = float("nan")
    mv[0, :, 2, 3] = 0.0                                                    # both land inside the frame, on their own pixels
    mv[0, :, 4, 4] = 0.0
    got = _backward(g, mv)
    assert bool(torch.isinf(got[0, 2, 3, 1])) and bool(torch.isnan(got[0, 4, 4, 2])) and bool(torch.isfinite(got[..., 0]).all())
    assert float(got[..., 0].abs().max()) > 0 and float(got[..., 3].abs().max()) > 0


def test_einval_before_any_launch():
    from cdfo_amd import _lib
    f = _lib.lib().cdfo_flow_warp_bwd_fixed
    x = torch.zeros(2 * 4 * 4 * 4, device="cuda")
    dx = torch.full((2 * 4 * 4 * 4,), float("nan"), device="cuda")
    acc, slots = torch.zeros(2 * 4 * 4 * 4, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    X, D, Ac, S, Z, s = p(x), p(dx), p(acc), p(slots), None, C.c_longlong(32)
    calls = [f(Z, 4, X, s, 2, 4, 4, 4, S, Ac, D, 4, None), f(X, 4, Z, s, 2, 4, 4, 4, S, Ac, D, 4, None), f(X, 4, X, s, 2, 4, 4, 4, Z, Ac, D, 4, None),
             f(X, 4, X, s, 2, 4, 4, 4, S, Z, D, 4, None), f(X, 4, X, s, 2, 4, 4, 4, S, Ac, Z, 4, None), f(X, 4, X, s, 0, 4, 4, 4, S, Ac, D, 4, None),
             f(X, 4, X, s, 2, 0, 4, 4, S, Ac, D, 4, None), f(X, 4, X, s, 2, 4, 0, 4, S, Ac, D, 4, None), f(X, 4, X, s, 2, 4, 4, 6, S, Ac, D, 8, None),
             f(X, 2, X, s, 2, 4, 4, 4, S, Ac, D, 4, None), f(X, 4, X, s, 2, 4, 4, 4, S, Ac, D, 2, None), f(X, 4, X, s, 2, 4, 4, 8, S, Ac, D, 4, None)]
    assert calls == [-1] * len(calls)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and not bool(acc.any())


def test_training_step_gives_equal_gradients_twice():
    """One `CVSR_V8` training step on fixed inputs and noise, twice: every parameter gradient has equal bits.  With the fp32 atomics of
    `cdfo_flow_warp_bwd` 39 of the 257 gradients differed between two such passes -- all of them upstream of the warp."""
    from arch.SIDECVSR_our import CVSR_V8
    from oracle.cvsr_v8_ref import make_inputs, make_state_dict
    dev = torch.device("cuda", 0)
    m = CVSR_V8()
    m.load_state_dict(make_state_dict(5), strict=True)
    m = m.to(dev).train()
    g = make_inputs(2, 16, 16, 56)
    hr = torch.rand(2, 1, 64, 64, generator=torch.Generator().manual_seed(9)).to(dev)

    def step():
        m.zero_grad(set_to_none=True)
        o, _ = m(g["x"].to(dev), None, g["mvs1"].to(dev), g["pms"].to(dev), g["rms"].to(dev), g["ufs"].to(dev),
                 gumbel_uniform=[u.to(dev) for u in g["gumbel_u"]])
        torch.sum(torch.sqrt((o - hr) ** 2 + 1e-4)).backward()
        return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}

    a, b = step(), step()
    differ = [k for k in a if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))]
    assert len(a) > 200 and not differ, differ[:8]
