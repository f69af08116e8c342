"""The operators only CVSR_V7 uses on the GPU, through their public wrappers (cdfo_amd.kernels) and autograd Functions
(cdfo_amd.cvsr_v7_train): csrc/v7_ops.hip and csrc/v7_train.hip.  Inputs, float64 references and bounds live in v7_cases.py;
test_v7_cases_cpu.py shows that those cases catch defective kernels.

How a kernel is held.  Real-valued results: max-abs error against float64 within fold_cases.bound = max(4 x the error of the same
definition in torch fp32 on the CPU, 2^-20 max|ref|), measured per case when the test runs -- no tolerance here is a constant.
Integer-valued data (the `ties` family of the per-pixel kernels, the integer families of shrink_planes and lincomb): equality.
The per-pixel kernels, the gate and the mix also run on rows of 128 channels read as [..., 64:128] (ld = 128), whose other half
holds 1e3.  Through the C interface, rdab_mix and spatial_gate write into NaN-filled pitched buffers with spare rows behind
them: padding and spare rows must stay NaN (a surplus wave of rdab_mix repeats the last tile, it does not write a tile of its own).
These, softmax64_bwd alone and the alignment check of cdfo_spatial_gate need the C interface (a pitched output, rows the Function
never passes, an entry point its wrapper guards); _lib.lib() sets every argtypes from include/cdfo_hip.h.

Each test prints its figures; the module prints every operator's worst error / bound with its case when it is done.
Measured on MI355X:
    operator                          cases   worst error / bound   error      bound      case
    T.chan_pool                          28                 0.042   5.03e-08   1.21e-06   negative-1-1-1
    T.chan_pool (exact)                  14   equal
    chan_pool                            28                 0.042   5.03e-08   1.21e-06   negative-1-1-1
    chan_pool (exact)                    14   equal
    chan_pool_bwd                        28                 0.045   1.04e-07   2.32e-06   plain-2-7-9
    chan_pool_bwd (exact)                14   equal
    dot_plane (dplane)                   28                 0.371   6.41e-07   1.73e-06   negative-1-1-1
    dot_plane (dplane) (exact)           14   equal
    gate_map_cumulative round 1           3                 0.179   6.62e-07   3.69e-06   7-2-9-11
    gate_map_cumulative round 2           3                 0.218   5.96e-07   2.73e-06   7-2-9-11
    gate_map_cumulative round 3           3                 0.221   5.14e-07   2.32e-06   7-2-9-11
    gate_map_cumulative round 4           3                 0.246   4.44e-07   1.80e-06   7-2-9-11
    gumbel_softmax extreme               14                 0.274   6.73e-07   2.46e-06   extreme-spread-1-7-9
    gumbel_softmax uniform               14                 0.250   3.11e-07   1.24e-06   uniform-spread-1-8-8
    lincomb                              18                 0.068   7.08e-07   1.03e-05   random-1028-False-True-new
    lincomb (exact)                      18   equal
    mul_plane                            28                 0.047   2.27e-07   4.79e-06   plain-1-4-4
    mul_plane (dx)                       28                 0.053   2.32e-07   4.37e-06   plain-2-7-9
    mul_plane (dx) (exact)               14   equal
    mul_plane (exact)                    14   equal
    rdab_mix extreme                     28                 0.279   3.17e-07   1.14e-06   extreme-peaked-3-1-1
    rdab_mix pitched output               7                 0.123   3.33e-07   2.71e-06   uniform-spread-1-7-9
    rdab_mix uniform                     28                 0.418   1.72e-06   4.12e-06   uniform-peaked-3-5-13
    shrink_planes level 1                 6                 0.065   4.47e-08   6.85e-07   random-2-2-16-24-1
    shrink_planes level 1 (exact)         6   equal
    shrink_planes level 2                 6                 0.069   1.49e-08   2.16e-07   random-1-1-4-4-2
    shrink_planes level 2 (exact)         6   equal
    softmax64_bwd + coldot (dv)          28                 0.360   1.46e-06   4.06e-06   extreme-peaked-3-5-13
    softmax64_bwd rows                   28                 0.164   1.00e-07   6.13e-07   plain-2-7-9
    spatial_gate 3x3                     14                 0.166   3.83e-09   2.30e-08   3-2-1-1
    spatial_gate 7x7                     14                 0.192   6.89e-07   3.59e-06   7-2-8-9
    spatial_gate 7x7 per-pixel shapes    14                 0.232   8.92e-07   3.85e-06   plain-3-12-20
    spatial_gate pitched output           7                 0.192   6.89e-07   3.59e-06   7-2-8-9
    the whole file: 320 tests in 3.6 s
No kernel fell outside its bound and no exact case failed.  The fast-intrinsic kernels (gate_map, gate_map_cumulative, rdab_mix with
__expf / __logf) use at most 0.42 of the bound, the `extreme` noise and the `peaked` v included; gumbel_softmax (expf / logf) 0.27.
"""
import ctypes as C

import pytest
import torch

import v7_cases as VC

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
WORST = {}                                   # operator -> (error / bound, error, bound, case id) of its worst case
CASES = {}                                   # operator -> comparisons made


def K():
    from cdfo_amd import kernels
    return kernels


def T():
    from cdfo_amd import cvsr_v7_train
    return cvsr_v7_train


def _error():
    from cdfo_amd._lib import CdfoError
    return CdfoError


def dev(t, pitch=False):
    """the tensor on the device; pitch: as [..., 64:128] of rows of 128 channels"""
    t = t.cuda().contiguous()
    return VC.pitched(t) if pitch else t


def _note(op, cid, ratio, err, tol):
    CASES[op] = CASES.get(op, 0) + 1
    if op not in WORST or ratio > WORST[op][0]:
        WORST[op] = (ratio, err, tol, cid)


def within(op, cid, got, ref, restated):
    """assert |got - ref| <= bound(ref, restated); NaN in `got` fails"""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (op, got.shape, ref.shape)
    tol = VC.bound(ref, restated)
    err = (got - ref).abs().max().item()
    print(f"{op} {cid}: err {err:.2e} bound {tol:.2e} ({err / tol:.3f}) max|ref| {ref.abs().max().item():.2e}")
    _note(op, cid, err / tol if err == err else float("inf"), err, tol)
    assert err <= tol, (op, cid, err, tol)


def same(op, cid, got, ref):
    got = got.detach().double().cpu()
    _note(op + " (exact)", cid, 0.0 if torch.equal(got, ref) else float("inf"), (got - ref).abs().max().item(), 0.0)
    assert torch.equal(got, ref), (op, cid, (got - ref).abs().max().item())


def held(op, cid, got, ref, restated, exact):
    same(op, cid, got, ref) if exact else within(op, cid, got, ref, restated)


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\noperator                          cases   worst error / bound   error      bound      case")
    for op in sorted(WORST):
        ratio, err, tol, cid = WORST[op]
        if op.endswith("(exact)"):
            print(f"{op:32s} {CASES[op]:6d}   {'equal' if ratio == 0.0 else 'NOT EQUAL: ' + cid}")
        else:
            print(f"{op:32s} {CASES[op]:6d} {ratio:21.3f}   {err:.2e}   {tol:.2e}   {cid}")


PITCHES = pytest.mark.parametrize("pitch", [False, True], ids=["dense", "ld128"])


# ------------------------------------------------------------------------------------------------------------ per-pixel kernels
@PITCHES
@pytest.mark.parametrize("c", VC.PIX_CASES, ids=VC.case_id)
def test_chan_pool_and_its_adjoint(c, pitch):
    d = VC.pix_inputs(c)
    exact, cid = c.family in VC.EXACT_FAMILIES, VC.case_id(c)
    (ref, gref), (r32, g32) = VC.pool_ref(c), VC.pool_ref(c, F32)
    held("chan_pool", cid, K().chan_pool(dev(d["x"], pitch)), ref, r32, exact)
    x = dev(d["x"], pitch).detach().requires_grad_()
    y = T().chan_pool(x)
    held("T.chan_pool", cid, y, ref, r32, exact)
    y.backward(dev(d["cot2"]))
    assert x.grad.shape == x.shape
    held("chan_pool_bwd", cid, x.grad, gref, g32, exact)


@PITCHES
@pytest.mark.parametrize("c", VC.PIX_CASES, ids=VC.case_id)
def test_mul_plane_and_both_gradients(c, pitch):
    d = VC.pix_inputs(c)
    exact, cid = c.family in VC.EXACT_FAMILIES, VC.case_id(c)
    x = dev(d["x"], pitch).detach().requires_grad_()
    plane = dev(d["plane"]).requires_grad_()
    out = T().mul_plane(x, plane)
    out.backward(dev(d["y"], pitch))
    ref, r32 = VC.mul_plane_ref(c), VC.mul_plane_ref(c, F32)
    held("mul_plane", cid, out, ref[0], r32[0], exact)
    held("mul_plane (dx)", cid, x.grad, ref[1], r32[1], exact)
    held("dot_plane (dplane)", cid, plane.grad, ref[2], r32[2], exact)


def _lib():
    from cdfo_amd import _lib as L
    return L.lib()


def _vp(t):
    return C.c_void_p(t.data_ptr())


@PITCHES
@pytest.mark.parametrize("c", [c for c in VC.PIX_CASES if c.family not in VC.EXACT_FAMILIES], ids=VC.case_id)
def test_softmax64_bwd_rows(c, pitch):
    """the kernel alone (the Function reaches it with dense rows and whole tiles only): npix from 1, rows and output of pitch 128"""
    (r, dz), (_, dz32) = VC.softmax_rows_ref(c), VC.softmax_rows_ref(c, F32)
    rows, dm = dev(r.float(), pitch), dev(VC.pix_inputs(c)["y"], pitch)
    out = dev(torch.full(r.shape, float("nan")), pitch)
    ld = VC.PITCH if pitch else 64
    assert c.B * c.H * c.W == 1 or rows.stride(-2) == dm.stride(-2) == out.stride(-2) == ld       # (one row has no pitch)
    status = _lib().cdfo_softmax64_bwd(_vp(rows), ld, _vp(dm), ld, C.c_longlong(c.B * c.H * c.W), _vp(out), ld, K()._stream())
    assert status == 0
    within("softmax64_bwd rows", VC.case_id(c), out, dz, dz32)
    if pitch:                                  # the rows' other half is nobody's to write
        assert (out._base[..., :64] == 1e3).all()


# ------------------------------------------------------------------------------------------------------------ pooled_conv users
@PITCHES
@pytest.mark.parametrize("c", VC.GATE_CASES, ids=VC.case_id)
def test_spatial_gate(c, pitch):
    x, w, b = VC.gate_inputs(c)
    out = K().spatial_gate(dev(x, pitch), dev(w), dev(b))
    within(f"spatial_gate {c.ks}x{c.ks}", VC.case_id(c), out, VC.gate_ref(c)[0], VC.gate_ref(c, F32)[0])


@PITCHES
@pytest.mark.parametrize("c", [c for c in VC.PIX_CASES if c.family == "plain"], ids=VC.case_id)
def test_spatial_gate_at_the_per_pixel_shapes(c, pitch):
    """spatial_gate_kernel holds 16 pixels per block like the per-pixel kernels: 1, 6, 15, 16, 17, 126 and 720 pixels"""
    x, w, b = VC.pix_gate_inputs(c)
    out = K().spatial_gate(dev(x, pitch), dev(w), dev(b))
    within("spatial_gate 7x7 per-pixel shapes", VC.case_id(c), out, VC.pix_gate_ref(c)[0], VC.pix_gate_ref(c, F32)[0])


@pytest.mark.parametrize("c", VC.CUM_CASES, ids=VC.case_id)
def test_gate_map_cumulative_is_spatial_attention_applied_four_times(c):
    """x_k = SpatialAttention(x_{k-1}) in float64 against x_0 G_k, the product formed in float64 from the kernel's plane"""
    x, w, b = VC.gate_inputs(c)
    pooled, G = K().chan_pool(dev(x)), None
    refs, refs32 = VC.cum_ref(c), VC.cum_ref(c, F32)
    for k in range(VC.CUM_ROUNDS):
        G = K().gate_map_cumulative(pooled, G, dev(w), dev(b))
        assert G.shape == x.shape[:3]
        within(f"gate_map_cumulative round {k + 1}", VC.case_id(c), x.double() * G.double().cpu().unsqueeze(-1), refs[k], refs32[k])


# ------------------------------------------------------------------------------------------------------------ rdab_mix, gumbel_softmax
@PITCHES
@pytest.mark.parametrize("c", VC.MIX_CASES, ids=VC.case_id)
def test_rdab_mix(c, pitch):
    d = VC.mix_inputs(c)
    out = K().rdab_mix(dev(d["xf"], pitch), dev(d["xc"], pitch), dev(d["w3"]), dev(d["b3"]), dev(d["v"]), dev(d["u"]))
    within(f"rdab_mix {c.noise}", VC.case_id(c), out, VC.mix_ref(c), VC.mix_ref(c, F32))


@pytest.mark.parametrize("c", VC.MIX_CASES, ids=VC.case_id)
def test_gumbel_softmax_and_its_gradient(c):
    d = VC.mix_inputs(c)
    v = dev(d["v"]).requires_grad_()
    r = T().gumbel_softmax(v, dev(d["u"]))
    r.backward(dev(d["cot"]))
    (ref, dv), (r32, dv32) = VC.softmax_ref(c), VC.softmax_ref(c, F32)
    within(f"gumbel_softmax {c.noise}", VC.case_id(c), r, ref, r32)
    within("softmax64_bwd + coldot (dv)", VC.case_id(c), v.grad, dv, dv32)


def _pitched_nans(c):
    """a NaN-filled [B P + 64, 128] buffer: rows of pitch 128 and a spare tile of rows behind the last image"""
    return torch.full((c.B * c.H * c.W + 64, VC.PITCH), float("nan"), dtype=torch.float32, device="cuda")


def _only_its_rows(buf, c):
    """the [B,H,W,64] result in a buffer of _pitched_nans; everything else must still be NaN"""
    n = c.B * c.H * c.W
    assert buf[:n, 64:].isnan().all() and buf[n:].isnan().all()
    return buf[:n, :64].reshape(c.B, c.H, c.W, 64)


@pytest.mark.parametrize("c", [c for c in VC.MIX_CASES if c.noise == "uniform" and c.v == "spread"], ids=VC.case_id)
def test_rdab_mix_writes_its_own_rows_only(c):
    d = {k: dev(t) for k, t in VC.mix_inputs(c).items()}
    buf = _pitched_nans(c)
    status = _lib().cdfo_rdab_mix(_vp(d["xf"]), 64, _vp(K().chan_pool(d["xc"])), _vp(d["w3"]), _vp(d["b3"]), _vp(d["v"]), _vp(d["u"]),
                                  c.B, c.H, c.W, _vp(buf), VC.PITCH, K()._stream())
    assert status == 0
    within("rdab_mix pitched output", VC.case_id(c), _only_its_rows(buf, c), VC.mix_ref(c), VC.mix_ref(c, F32))


@pytest.mark.parametrize("c", [c for c in VC.GATE_CASES if c.ks == 7], ids=VC.case_id)
def test_spatial_gate_writes_its_own_rows_only(c):
    x, w, b = (dev(t) for t in VC.gate_inputs(c))
    buf = _pitched_nans(c)
    gate = torch.empty(c.B * c.H * c.W, dtype=torch.float32, device="cuda")
    status = _lib().cdfo_spatial_gate(_vp(x), 64, _vp(K().chan_pool(x)), _vp(w), _vp(b), c.B, c.H, c.W, 64, c.ks, _vp(gate), _vp(buf),
                                      VC.PITCH, K()._stream())
    assert status == 0
    within("spatial_gate pitched output", VC.case_id(c), _only_its_rows(buf, c), VC.gate_ref(c)[0], VC.gate_ref(c, F32)[0])


# ------------------------------------------------------------------------------------------------------------ shrink_planes
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "frame_of_7"])
@pytest.mark.parametrize("c", VC.SHRINK_CASES, ids=VC.case_id)
def test_shrink_planes(c, strided):
    t = VC.shrink_input(c).cuda()
    src = t[:, VC.SHRINK_FRAME]
    assert src.stride(0) == VC.SHRINK_FRAMES * c.planes * c.H * c.W
    out = K().shrink_planes(src if strided else src.contiguous(), c.level)
    held(f"shrink_planes level {c.level}", VC.case_id(c), out, VC.shrink_ref(c), VC.shrink_ref(c, F32), c.data == "integer")


# ------------------------------------------------------------------------------------------------------------ lincomb
@pytest.mark.parametrize("c", VC.LIN_CASES, ids=VC.case_id)
def test_lincomb(c):
    a, b, cc_ = (t.cuda() for t in VC.lin_inputs(c))
    ca, cb, cc = VC.LIN_COEFFS[c.data]
    out = {"new": None, "a": a, "b": b}[c.out]
    got = K().lincomb(a, ca, b if c.has_b else None, cb, cc_ if c.has_c else None, cc, out=out)
    assert out is None or got is out
    held("lincomb", VC.case_id(c), got, VC.lin_ref(c), VC.lin_ref(c, F32), c.data == "integer")
    if c.out != "a":
        assert torch.equal(a.cpu(), VC.lin_inputs(c)[0])          # the operands that are not the output are left alone
    assert torch.equal(cc_.cpu(), VC.lin_inputs(c)[2])


# ------------------------------------------------------------------------------------------------------------ the error surface
def test_shrink_planes_refuses_sizes_and_levels_it_cannot_serve():
    z = torch.zeros(1, 1, 8, 8, device="cuda")
    for t, level in ((z[..., :6, :], 2), (z[..., :6], 2), (z[..., :7, :], 1), (z[..., :7], 1), (z, 3), (z, 0)):
        with pytest.raises(_error()):
            K().shrink_planes(t.contiguous(), level)
    assert K().shrink_planes(z, 2).shape == (1, 1, 2, 2)


def test_lincomb_refuses_a_length_that_is_no_multiple_of_4():
    a = torch.zeros(6, device="cuda")
    with pytest.raises(_error()):
        K().lincomb(a, 1.0, a.clone(), 1.0)
    with pytest.raises(ValueError):
        K().lincomb(torch.zeros(8, device="cuda"), 1.0, torch.zeros(4, device="cuda"), 1.0)


def test_chan_pool_refuses_32_channels():
    with pytest.raises(_error()):
        K().chan_pool(torch.zeros(1, 2, 2, 32, device="cuda"))


def test_rdab_mix_refuses_noise_it_would_misread():
    c = VC.MixCase("uniform", "spread", 1, 5, 13)
    d = {k: dev(t) for k, t in VC.mix_inputs(c).items()}
    args = lambda u: (d["xf"], d["xc"], d["w3"], d["b3"], d["v"], u)  # noqa: E731
    nhwc_noise = d["u"].permute(0, 2, 3, 1).contiguous()
    for u in (nhwc_noise.permute(0, 3, 1, 2),           # the right shape, not contiguous
              nhwc_noise,                               # [B,H,W,64]
              d["u"][:, :32].contiguous(), d["u"].transpose(2, 3).contiguous(), d["u"].double()):
        with pytest.raises(ValueError):
            K().rdab_mix(*args(u))
    with pytest.raises(ValueError):
        K().rdab_mix(d["xf"], d["xc"], d["w3"], d["b3"], d["v"].view(64, 1), d["u"])


def test_a_view_that_is_not_16_byte_aligned_is_refused():
    """[..., 1:65] of rows of 128 channels starts 4 bytes into a row: the float4 kernels cannot read it, the wrappers and the
    Functions say so instead of reading beside it"""
    c = VC.PixCase("plain", 2, 7, 9)
    d = VC.pix_inputs(c)
    wide = torch.zeros(c.B, c.H, c.W, VC.PITCH, device="cuda")
    wide[..., 1:65] = d["x"].cuda()
    x = wide[..., 1:65]
    assert x.data_ptr() % 16 == 4
    w, b = torch.zeros(1, 2, 3, 3, device="cuda"), torch.zeros(1, device="cuda")
    good = x.contiguous()                      # an aligned copy: rdab_mix pools xc first, so only xf may be the view
    v, u = torch.zeros(c.B, 64, device="cuda"), torch.full((c.B, 64, c.H, c.W), 0.5, device="cuda")
    for call in (lambda: K().chan_pool(x), lambda: K().spatial_gate(x, w, b), lambda: T().chan_pool(x),
                 lambda: T().mul_plane(x, dev(d["plane"])), lambda: K().rdab_mix(x, good, w, b, v, u)):
        with pytest.raises(_error()):
            call()
    assert K().rdab_mix(good, good, w, b, v, u).shape == good.shape          # ... and nothing else about that call was wrong
    # K.spatial_gate pools x before it reaches cdfo_spatial_gate: that entry point's own checks, with the pooled map of the copy
    pooled, gate = K().chan_pool(good), torch.empty(c.B * c.H * c.W, device="cuda")
    out, wide_out = torch.empty_like(good), torch.zeros_like(wide)
    call = lambda src, ld, dst, ldo: _lib().cdfo_spatial_gate(_vp(src), ld, _vp(pooled), _vp(w), _vp(b), c.B, c.H, c.W, 64, 3,  # noqa: E731
                                                              _vp(gate), _vp(dst), ldo, K()._stream())
    EALIGN = -2
    assert call(x, VC.PITCH, out, 64) == EALIGN and call(good, 64, wide_out[..., 1:65], VC.PITCH) == EALIGN
    assert call(good, 64, out, 64) == 0 and wide_out.abs().max().item() == 0.0
