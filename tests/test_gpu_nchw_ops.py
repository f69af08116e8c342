"""The small NCHW operators of the DCN consumers on the GPU, entry point by entry point (csrc/nchw_ops.hip, csrc/nchw_bwd.hip), and
the two layout transposes of csrc/layout.hip.  Inputs, float64 references and bounds live in nchw_cases.py;
test_nchw_cases_cpu.py shows that those cases catch defective kernels.

How a kernel is held.  Every output buffer is pre-filled with NaN (an unwritten element shows), pitched outputs must leave
their padding NaN.  Real-valued results: max-abs error against float64 within fold_cases.bound = max(4 x the error of the
same formula in torch fp32 on the CPU, 2^-20 max|ref|), measured per case when the test runs.  Integer-valued data (max-pool
forward and routing, the zeros of rows no window reaches, the layout changes): equality.  Every backward runs twice and must give
equal bits.  The LINEAR operators are also tied to the project's own forward by the dot test in float64, <op(x), g> against
<x, bwd(g)>: both sides are sums of products of one within-bound tensor and one exact tensor, so they may differ by at most
bound(op) sum|g| + bound(bwd) sum|x|.  The non-linear ones (relu / sigmoid / the gate in a, the offset / mask assembly in o1,
o2) have no such identity; they are held by float64 autograd alone.

Measured on MI355X (error .. bound, worst error / bound over the cases of a row); each test prints its own figures:
    conv2d none                         14 cases  err 1.91e-07 .. 1.00e-06   bound 2.12e-06 .. 6.96e-06   worst 0.246
    conv2d relu                         14 cases  err 5.91e-08 .. 8.36e-07   bound 8.13e-07 .. 6.96e-06   worst 0.194
    conv2d sigmoid                      14 cases  err 3.94e-08 .. 1.21e-07   bound 6.69e-07 .. 9.53e-07   worst 0.128
    conv2d grid                          1 cases  err 4.77e-07 .. 4.77e-07   bound 1.13e-05 .. 1.13e-05   worst 0.042
    conv2d_bwd gin                      14 cases  err 1.16e-07 .. 1.79e-06   bound 1.81e-06 .. 1.11e-05   worst 0.322
    conv2d_bwd gw                       14 cases  err 2.21e-07 .. 3.16e-06   bound 5.30e-06 .. 3.95e-05   worst 0.109
    conv2d_bwd gbias                    14 cases  err 1.19e-07 .. 1.98e-06   bound 2.41e-06 .. 3.55e-05   worst 0.152
    conv2d_bwd bias only                 2 cases  err 1.19e-07 .. 1.71e-06   bound 2.41e-06 .. 1.53e-05   worst 0.111
    resize                               6 cases  err 0.00e+00 .. 2.60e-07   bound 1.12e-06 .. 2.55e-06   worst 0.102
    resize accumulate                    6 cases  err 3.73e-08 .. 3.50e-07   bound 1.87e-06 .. 4.94e-06   worst 0.071
    resize grid                          1 cases  err 5.26e-07 .. 5.26e-07   bound 3.99e-06 .. 3.99e-06   worst 0.132
    resize_bwd                           6 cases  err 0.00e+00 .. 3.17e-06   bound 5.20e-07 .. 1.54e-05   worst 0.205
    ew mode 0                            5 cases  err 1.19e-07 .. 4.77e-07   bound 3.61e-06 .. 9.65e-06   worst 0.049
    ew mode 1                            5 cases  err 0.00e+00 .. 0.00e+00   bound 1.17e-06 .. 7.63e-06   worst 0.000
    ew mode 2                            5 cases  err 3.86e-08 .. 8.75e-08   bound 7.37e-07 .. 9.53e-07   worst 0.092
    ew mode 3                            5 cases  err 6.69e-08 .. 1.76e-07   bound 9.57e-07 .. 2.44e-06   worst 0.122
    ew_bwd mode 1                        5 cases  err 0.00e+00 .. 0.00e+00   bound 1.96e-06 .. 3.55e-06   worst 0.000
    ew_bwd mode 2                        5 cases  err 1.18e-08 .. 8.53e-08   bound 3.45e-07 .. 7.90e-07   worst 0.108
    ew_bwd mode 4                        5 cases  err 0.00e+00 .. 1.66e-09   bound 3.20e-10 .. 1.73e-06   worst 0.052
    ew_bwd mode 5                        5 cases  err 4.12e-08 .. 1.84e-07   bound 4.47e-07 .. 7.74e-07   worst 0.240
    ew_bwd mode 6                        5 cases  err 6.07e-08 .. 1.50e-07   bound 1.35e-06 .. 2.05e-06   worst 0.096
    avgpool                              5 cases  err 0.00e+00 .. 3.68e-08   bound 2.52e-07 .. 1.40e-06   worst 0.109
    gate_bwd_y                           5 cases  err 2.04e-07 .. 1.06e-05   bound 2.22e-06 .. 8.92e-05   worst 0.119
    ew mode 3 grid                       1 cases  err 4.49e-07 .. 4.49e-07   bound 4.95e-06 .. 4.95e-06   worst 0.091
    ew_bwd mode 5 grid                   1 cases  err 5.95e-07 .. 5.95e-07   bound 2.82e-06 .. 2.82e-06   worst 0.211
    mv_offset_mask offset               24 cases  err 2.34e-06 .. 3.01e-06   bound 2.47e-05 .. 3.05e-05   worst 0.120
    mv_offset_mask mask                 24 cases  err 8.07e-08 .. 9.32e-08   bound 9.53e-07 .. 9.53e-07   worst 0.098
    mv_offset_mask_bwd g1               24 cases  err 2.05e-06 .. 4.67e-06   bound 2.29e-05 .. 4.46e-05   worst 0.125
    mv_offset_mask_bwd g2               24 cases  err 2.31e-06 .. 4.72e-06   bound 2.78e-05 .. 3.83e-05   worst 0.130
    through nchw_autograd (conv2d x 3 activations, resize, relu, sigmoid, add, gate, plane_mean, offset_mask): 52 comparisons, worst 0.232
    dot tests (conv in x and in w, resize, plane mean, gate in x and in yv): 49, worst |difference| / bound 0.018
    max-pool forward and routing (16 cases each), zeros of unreached rows, layout (20 shapes x 2 pitches), repeated backwards: exact
    the whole file: 236 tests in 4.8 s
No case needed the allowance for a fast-math exponential (conv2d's sigmoid is __expf: worst 0.128).  The resize rows are against
fused source positions (nchw_cases.resize_taps); against positions with the product rounded first the 87 -> 520 case read
2.18e-05 / 3.99e-06 = 5.47, the same excess as F.interpolate on the CPU (5.50): the reference was wrong, not the kernel.
With the parent's library the NaN cases of test_maxpool and both cases of test_conv2d_bwd_bias_only_fills_a_nan_prefilled_gbias fail.
"""
import ctypes as C

import pytest
import torch

import nchw_cases as NC

pytestmark = pytest.mark.gpu
NAN = float("nan")
EINVAL = -1


def _lib():
    from cdfo_amd import _lib as L
    return L.lib()


def _stream():
    from cdfo_amd import kernels as K
    return K._stream()


def _act_code(name):
    from cdfo_amd import kernels as K
    return {"none": K.ACT_NONE, "relu": K.ACT_RELU, "sigmoid": K.ACT_SIGMOID}[name]


def vp(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def dev(t):
    return None if t is None else t.cuda().contiguous()


def nans(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def ok(status):
    assert status == 0, status


def _report(what, got, ref, tol):
    got = got.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    print(f"{what}: err {err:.2e} bound {tol:.2e} ({err / tol:.3f}) max|ref| {ref.abs().max().item():.2e}")
    return err


def _within(what, got, ref, restated):
    """assert |got - ref| <= bound(ref, restated); NaN in `got` fails.  Returns the bound."""
    tol = NC.bound(ref, restated)
    err = _report(what, got, ref, tol)
    assert err <= tol, (what, err, tol)
    return tol


def _dot(what, lhs_a, lhs_b, rhs_a, rhs_b, tol_l, tol_r):
    """<lhs_a, lhs_b> against <rhs_a, rhs_b>: lhs_a and rhs_b come from the device (within tol_l / tol_r of the truth), lhs_b
    and rhs_a are exact inputs."""
    la, lb, ra, rb = (t.double().cpu().flatten() for t in (lhs_a, lhs_b, rhs_a, rhs_b))
    lhs, rhs = (la * lb).sum().item(), (ra * rb).sum().item()
    tol = tol_l * lb.abs().sum().item() + tol_r * ra.abs().sum().item()
    print(f"{what}: dot test {lhs:.9g} vs {rhs:.9g}, |diff| {abs(lhs - rhs):.2e} bound {tol:.2e}")
    assert abs(lhs - rhs) <= tol, (what, lhs, rhs, tol)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------ conv2d
def _conv(c, x, w, b, act="none"):
    Ho, Wo = NC.conv_out_hw(c)
    out = nans(c.B, c.Co, Ho, Wo)
    ok(_lib().cdfo_conv2d_nchw(vp(x), vp(w), vp(b), c.B, c.C, c.H, c.W, c.Co, c.k, c.k, c.stride, c.pad, _act_code(act), vp(out),
                               _stream()))
    return out


def _conv_bwd(c, x, w, g, gin=True, gw=True, gb=True):
    outs = (nans(c.B, c.C, c.H, c.W) if gin else None, nans(c.Co, c.C, c.k, c.k) if gw else None, nans(c.Co) if gb else None)
    ok(_lib().cdfo_conv2d_nchw_bwd(vp(x), vp(w), vp(g), c.B, c.C, c.H, c.W, c.Co, c.k, c.k, c.stride, c.pad, vp(outs[0]), vp(outs[1]),
                                   vp(outs[2]), _stream()))
    return outs


@pytest.mark.parametrize("act", NC.ACTS)
@pytest.mark.parametrize("c", NC.CONV_CASES, ids=NC.case_id)
def test_conv2d(c, act):
    x, w, b, _ = NC.conv_inputs(c)
    out = _conv(c, dev(x), dev(w), dev(b), act)
    _within(f"conv2d {NC.case_id(c)} {act}", out, NC.conv_ref(c, act), NC.conv_ref(c, act, torch.float32))


def test_conv2d_grid_stride():
    """4 326 400 outputs on a grid capped at 4 194 304 threads: the second trip, the last element."""
    c = NC.CONV_GRID_CASE
    x, w, b, _ = NC.conv_inputs(c)
    out = _conv(c, dev(x), dev(w), dev(b))
    ref = NC.conv_ref(c)
    assert ref.numel() > NC.GRID_CAP
    tol = _within("conv2d grid", out, ref, NC.conv_ref(c, dtype=torch.float32))
    assert abs(out.flatten()[-1].item() - ref.flatten()[-1].item()) <= tol


@pytest.mark.parametrize("c", NC.CONV_CASES, ids=NC.case_id)
def test_conv2d_bwd(c):
    x, w, b, g = NC.conv_inputs(c)
    xd, wd, gd = dev(x), dev(w), dev(g)
    gin, gw, gb = _conv_bwd(c, xd, wd, gd)
    again = _conv_bwd(c, xd, wd, gd)
    name = f"conv2d_bwd {NC.case_id(c)}"
    ref, ref32 = NC.conv_grad_ref(c), NC.conv_grad_ref(c, dtype=torch.float32)
    tols = [_within(f"{name} {what}", got, r, r32) for what, got, r, r32 in zip(("gin", "gw", "gbias"), (gin, gw, gb), ref, ref32)]
    for a, bb in zip((gin, gw, gb), again):
        assert torch.equal(_bits(a), _bits(bb))
    if c.name == "unused_edge":
        assert (gin[:, :, -1, :] == 0).all() and (gin[:, :, :, -1] == 0).all() and (gin[:, :, :-1, :-1] != 0).any()
    # the linear part (no bias) of the project's own forward
    out = _conv(c, xd, wd, None)
    lin, lin32 = NC.conv_ref(c, bias=False), NC.conv_ref(c, dtype=torch.float32, bias=False)
    tol_out = NC.bound(lin, lin32)
    _dot(f"{name} in x", out, g, x, gin, tol_out, tols[0])
    _dot(f"{name} in w", out, g, w, gw, tol_out, tols[1])


@pytest.mark.parametrize("c", (NC.CONV_CASES[3], NC.CONV_CASES[-2]), ids=NC.case_id)
def test_conv2d_bwd_bias_only_fills_a_nan_prefilled_gbias(c):
    """gbias without gw (and without `in`): computed, the same bits as with gw; gin alone and gw alone are complete too."""
    x, w, b, g = NC.conv_inputs(c)
    xd, wd, gd = dev(x), dev(w), dev(g)
    full = _conv_bwd(c, xd, wd, gd)
    gb = nans(c.Co)
    ok(_lib().cdfo_conv2d_nchw_bwd(None, None, vp(gd), c.B, c.C, c.H, c.W, c.Co, c.k, c.k, c.stride, c.pad, None, None, vp(gb), _stream()))
    ref, ref32 = NC.conv_grad_ref(c), NC.conv_grad_ref(c, dtype=torch.float32)
    _within(f"conv2d_bwd bias only {NC.case_id(c)}", gb, ref[2], ref32[2])
    assert torch.equal(_bits(gb), _bits(full[2]))
    only_gin = _conv_bwd(c, None, wd, gd, gw=False, gb=False)[0]
    only_gw = _conv_bwd(c, xd, None, gd, gin=False, gb=False)[1]
    assert torch.equal(_bits(only_gin), _bits(full[0])) and torch.equal(_bits(only_gw), _bits(full[1]))


@pytest.mark.parametrize("c", (NC.CONV_CASES[3], NC.CONV_CASES[6], NC.CONV_CASES[-1]), ids=NC.case_id)
def test_conv2d_autograd(c):
    """nchw_autograd.conv2d under torch autograd, all three activations (their gradients are cdfo_ew_nchw_bwd modes 1 and 2 on
    the saved output); then the bias as the only leaf."""
    from cdfo_amd import nchw_autograd as A
    x, w, b, g = NC.conv_inputs(c)
    for act in NC.ACTS:
        leaves = [t.cuda().requires_grad_() for t in (x, w) + ((b,) if c.bias else ())]
        y = A.conv2d(leaves[0], leaves[1], leaves[2] if c.bias else None, c.stride, c.pad, _act_code(act))
        name = f"autograd conv2d {NC.case_id(c)} {act}"
        _within(name, y.detach(), NC.conv_ref(c, act), NC.conv_ref(c, act, torch.float32))
        y.backward(g.cuda())
        for what, leaf, r, r32 in zip(("gin", "gw", "gbias"), leaves, NC.conv_grad_ref(c, act), NC.conv_grad_ref(c, act, torch.float32)):
            _within(f"{name} {what}", leaf.grad, r, r32)
    if c.bias:
        bias = b.cuda().requires_grad_()
        A.conv2d(x.cuda(), w.cuda(), bias, c.stride, c.pad, _act_code("none")).backward(g.cuda())
        _within(f"autograd conv2d {NC.case_id(c)} bias leaf", bias.grad, NC.conv_grad_ref(c)[2], NC.conv_grad_ref(c, dtype=torch.float32)[2])


# ------------------------------------------------------------------------------------------------------------ max-pool
def _pool(c, x):
    Ho, Wo = NC.pool_out_hw(c)
    # where NaN is an expected result, an unwritten element has to look different: -7 is no value of the inputs
    out = nans(c.B, c.C, Ho, Wo) if c.data != "nan" else torch.full((c.B, c.C, Ho, Wo), -7.0, device="cuda")
    ok(_lib().cdfo_maxpool_nchw(vp(x), c.B * c.C, c.H, c.W, c.k, c.stride, vp(out), _stream()))
    return out


def _pool_bwd(c, x, g):
    gin = nans(c.B, c.C, c.H, c.W)
    idx = torch.full((g.numel(),), -1, dtype=torch.int32, device="cuda")
    ok(_lib().cdfo_maxpool_nchw_bwd(vp(x), vp(g), c.B * c.C, c.H, c.W, c.k, c.stride, vp(idx), vp(gin), _stream()))
    return gin


@pytest.mark.parametrize("c", NC.POOL_CASES, ids=NC.case_id)
def test_maxpool(c):
    """Exact; a NaN anywhere in a window gives NaN, as F.max_pool2d and the project's own arg-max do."""
    x, _ = NC.pool_inputs(c)
    out = _pool(c, dev(x))
    ref, _ = NC.pool_ref(c)
    if c.data == "nan":
        assert ref[0, :, 0, 0].isnan().all()
    assert NC.same_with_nan(out, ref), (out.cpu(), ref)


@pytest.mark.parametrize("c", NC.POOL_CASES, ids=NC.case_id)
def test_maxpool_bwd(c):
    """Exact routing: ties to the first maximum in scan order, a NaN tap wins, rows and columns past the last window get 0."""
    x, g = NC.pool_inputs(c)
    xd, gd = dev(x), dev(g)
    gin = _pool_bwd(c, xd, gd)
    _, ref = NC.pool_ref(c)
    assert torch.equal(gin.double().cpu(), ref), (gin.cpu(), ref)
    assert torch.equal(_bits(gin), _bits(_pool_bwd(c, xd, gd)))
    Ho, Wo = NC.pool_out_hw(c)
    ry, rx = (Ho - 1) * c.stride + c.k, (Wo - 1) * c.stride + c.k
    assert (gin[:, :, ry:, :] == 0).all() and (gin[:, :, :, rx:] == 0).all()
    if c.data in ("distinct", "ties"):           # sum out g == sum x gin, in integers
        out = _pool(c, xd)
        assert (out.double() * gd.double()).sum().item() == (xd.double() * gin.double()).sum().item()


def test_maxpool_autograd():
    from cdfo_amd import nchw_autograd as A
    c = NC.POOL_CASES[5]
    x, g = NC.pool_inputs(c)
    xd = x.cuda().requires_grad_()
    y = A.maxpool(xd, c.k, c.stride)
    y.backward(g.cuda())
    ref, gref = NC.pool_ref(c)
    assert torch.equal(y.detach().double().cpu(), ref) and torch.equal(xd.grad.double().cpu(), gref)


# ------------------------------------------------------------------------------------------------------------ bilinear resize
def _resize(c, x, out=None, accumulate=0):
    out = nans(c.B, c.C, c.Ho, c.Wo) if out is None else out
    ok(_lib().cdfo_resize_bilinear_nchw(vp(x), c.B * c.C, c.H, c.W, c.Ho, c.Wo, accumulate, vp(out), _stream()))
    return out


def _resize_bwd(c, g):
    gin = nans(c.B, c.C, c.H, c.W)
    ok(_lib().cdfo_resize_bilinear_nchw_bwd(vp(g), c.B * c.C, c.H, c.W, c.Ho, c.Wo, vp(gin), _stream()))
    return gin


@pytest.mark.parametrize("c", NC.RESIZE_CASES, ids=NC.case_id)
def test_resize_bilinear(c):
    x, _, out0 = NC.resize_inputs(c)
    name = f"resize {NC.case_id(c)}"
    ref, ref32 = NC.resize_ref(c), NC.resize_ref(c, torch.float32)
    _within(name, _resize(c, dev(x)), ref, ref32)
    acc = _resize(c, dev(x), out0.cuda().clone(), 1)
    _within(name + " accumulate", acc, ref + out0.double(), ref32 + out0)
    if (c.H, c.W) == (c.Ho, c.Wo):
        assert torch.equal(_resize(c, dev(x)).cpu(), x)


def test_resize_bilinear_grid_stride():
    c = NC.RESIZE_GRID_CASE
    x = NC.resize_inputs(c)[0]
    out = _resize(c, dev(x))
    ref = NC.resize_ref(c)
    assert ref.numel() > NC.GRID_CAP
    tol = _within("resize grid", out, ref, NC.resize_ref(c, torch.float32))
    assert abs(out.flatten()[-1].item() - ref.flatten()[-1].item()) <= tol


@pytest.mark.parametrize("c", NC.RESIZE_CASES, ids=NC.case_id)
def test_resize_bilinear_bwd(c):
    x, g, _ = NC.resize_inputs(c)
    gd = dev(g)
    gin = _resize_bwd(c, gd)
    name = f"resize_bwd {NC.case_id(c)}"
    tol_g = _within(name, gin, NC.resize_grad_ref(c), NC.resize_grad_ref(c, torch.float32))
    assert torch.equal(_bits(gin), _bits(_resize_bwd(c, gd)))
    _dot(name, _resize(c, dev(x)), g, x, gin, NC.bound(NC.resize_ref(c), NC.resize_ref(c, torch.float32)), tol_g)


def test_resize_autograd():
    from cdfo_amd import nchw_autograd as A
    c = NC.RESIZE_CASES[2]
    x, g, _ = NC.resize_inputs(c)
    xd = x.cuda().requires_grad_()
    y = A.resize_bilinear(xd, c.Ho, c.Wo)
    y.backward(g.cuda())
    _within("autograd resize", y.detach(), NC.resize_ref(c), NC.resize_ref(c, torch.float32))
    _within("autograd resize gin", xd.grad, NC.resize_grad_ref(c), NC.resize_grad_ref(c, torch.float32))


# ------------------------------------------------------------------------------------------------------------ plane mean, element-wise modes, gate
def _ew(c, mode, d):
    out = nans(c.B, c.C, c.H, c.W)
    need = {0: ("b",), 1: (), 2: (), 3: ("x", "yv")}[mode]
    ok(_lib().cdfo_ew_nchw(vp(d["a"]), vp(d["b"] if "b" in need else None), vp(d["x"] if "x" in need else None),
                           vp(d["yv"] if "yv" in need else None), out.numel(), c.H * c.W, mode, vp(out), _stream()))
    return out


def _ew_bwd(c, mode, d):
    out = nans(c.B, c.C, c.H, c.W)
    g = d["gp"] if mode == 4 else d["g"]
    y = d["y_relu"] if mode == 1 else d["y_sigmoid"] if mode == 2 else None
    a, x, yv = (d["a"], d["x"] if mode == 5 else None, d["yv"]) if mode in (5, 6) else (None, None, None)
    ok(_lib().cdfo_ew_nchw_bwd(vp(g), vp(y), vp(a), vp(x), vp(yv), out.numel(), c.H * c.W, mode, vp(out), _stream()))
    return out


def _mean(c, x):
    out = nans(c.B, c.C, 1, 1)
    ok(_lib().cdfo_avgpool_nchw(vp(x), c.B * c.C, c.H * c.W, vp(out), _stream()))
    return out


def _gate_y(c, d):
    out = nans(c.B, c.C, 1, 1)
    ok(_lib().cdfo_gate_nchw_bwd_y(vp(d["g"]), vp(d["a"]), vp(d["x"]), c.B * c.C, c.H * c.W, vp(out), _stream()))
    return out


def _ew_dev(c):
    return {k: v.cuda() for k, v in NC.ew_inputs(c).items()}


@pytest.mark.parametrize("mode", NC.EW_MODES)
@pytest.mark.parametrize("c", NC.EW_CASES, ids=NC.case_id)
def test_ew(c, mode):
    out = _ew(c, mode, _ew_dev(c))
    ref = NC.ew_ref(c, mode)
    if mode in (0, 1):
        assert torch.equal(out.double().cpu(), NC.ew_ref(c, mode, torch.float32).double())       # one rounding, or none
    _within(f"ew mode {mode} {NC.case_id(c)}", out, ref, NC.ew_ref(c, mode, torch.float32))


@pytest.mark.parametrize("mode", NC.EW_BWD_MODES)
@pytest.mark.parametrize("c", NC.EW_CASES, ids=NC.case_id)
def test_ew_bwd(c, mode):
    d = _ew_dev(c)
    out = _ew_bwd(c, mode, d)
    name = f"ew_bwd mode {mode} {NC.case_id(c)}"
    tol = _within(name, out, NC.ew_bwd_ref(c, mode), NC.ew_bwd_ref(c, mode, torch.float32))
    assert torch.equal(_bits(out), _bits(_ew_bwd(c, mode, d)))
    host = NC.ew_inputs(c)
    if mode == 4:       # adjoint of the plane mean
        _dot(name, _mean(c, d["x"]), host["gp"], host["x"], out, NC.bound(NC.mean_ref(c), NC.mean_ref(c, torch.float32)), tol)
    if mode == 6:       # the gate is linear in x
        _dot(name, _ew(c, 3, d), host["g"], host["x"], out, NC.bound(NC.ew_ref(c, 3), NC.ew_ref(c, 3, torch.float32)), tol)


@pytest.mark.parametrize("c", NC.EW_CASES, ids=NC.case_id)
def test_avgpool(c):
    _within(f"avgpool {NC.case_id(c)}", _mean(c, dev(NC.ew_inputs(c)["x"])), NC.mean_ref(c), NC.mean_ref(c, torch.float32))


@pytest.mark.parametrize("c", NC.EW_CASES, ids=NC.case_id)
def test_gate_bwd_y(c):
    d = _ew_dev(c)
    out = _gate_y(c, d)
    name = f"gate_bwd_y {NC.case_id(c)}"
    tol = _within(name, out, NC.gate_grads(c)[2], NC.gate_grads(c, torch.float32)[2])
    assert torch.equal(_bits(out), _bits(_gate_y(c, d)))
    host = NC.ew_inputs(c)    # the gate is linear in yv
    _dot(name, _ew(c, 3, d), host["g"], host["yv"], out, NC.bound(NC.ew_ref(c, 3), NC.ew_ref(c, 3, torch.float32)), tol)


def test_ew_grid_stride():
    """ew (the gate, mode 3) and ew_bwd (mode 5) on 4 326 400 elements: the second trip of the capped grid, the last element."""
    c = NC.EW_GRID_CASE
    d = _ew_dev(c)
    assert d["a"].numel() > NC.GRID_CAP
    for what, out, ref, ref32 in (("ew mode 3", _ew(c, 3, d), NC.ew_ref(c, 3), NC.ew_ref(c, 3, torch.float32)),
                                  ("ew_bwd mode 5", _ew_bwd(c, 5, d), NC.ew_bwd_ref(c, 5), NC.ew_bwd_ref(c, 5, torch.float32))):
        tol = _within(what + " grid", out, ref, ref32)
        assert abs(out.flatten()[-1].item() - ref.flatten()[-1].item()) <= tol


def test_ew_autograd():
    """plane_mean, relu, sigmoid, add and gate of nchw_autograd under torch autograd."""
    from cdfo_amd import nchw_autograd as A
    c = NC.EW_CASES[3]
    h = NC.ew_inputs(c)
    a, b, x, yv = (h[k].cuda().requires_grad_() for k in ("a", "b", "x", "yv"))
    y = A.gate(A.add(a, b), x, yv)
    y.backward(h["g"].cuda())
    d = {k: v.double() for k, v in h.items()}
    for dtype in (torch.float64, torch.float32):
        leaves = [h[k].to(dtype).clone().requires_grad_() for k in ("a", "b", "x", "yv")]
        yr = leaves[2] * torch.sigmoid(leaves[0] + leaves[1]) * leaves[3]
        res = (yr.detach(),) + torch.autograd.grad((yr * h["g"].to(dtype)).sum(), leaves)
        if dtype == torch.float64:
            ref = res
    for what, got, r, r32 in zip(("out", "ga", "gb", "gx", "gyv"), (y.detach(), a.grad, b.grad, x.grad, yv.grad), ref, res):
        _within(f"autograd gate(add) {what}", got, r, r32)
    for fn, mode in ((A.relu, 1), (A.sigmoid, 2)):
        a = h["a"].cuda().requires_grad_()
        y = fn(a)
        y.backward(h["g"].cuda())
        _within(f"autograd mode {mode}", y.detach(), NC.ew_ref(c, mode), NC.ew_ref(c, mode, torch.float32))
        ar = d["a"].clone().requires_grad_()
        gr = torch.autograd.grad((NC._act(ar, "relu" if mode == 1 else "sigmoid") * d["g"]).sum(), ar)[0]
        a32 = h["a"].clone().requires_grad_()
        g32 = torch.autograd.grad((NC._act(a32, "relu" if mode == 1 else "sigmoid") * h["g"]).sum(), a32)[0]
        _within(f"autograd mode {mode} ga", a.grad, gr, g32)
    x = h["x"].cuda().requires_grad_()
    m = A.plane_mean(x)
    m.backward(h["gp"].cuda())
    _within("autograd plane_mean", m.detach(), NC.mean_ref(c), NC.mean_ref(c, torch.float32))
    _within("autograd plane_mean gx", x.grad, NC.ew_bwd_ref(c, 4), NC.ew_bwd_ref(c, 4, torch.float32))


# ------------------------------------------------------------------------------------------------------------ offset / mask assembly
def _om(c, o1, o2, flow):
    ld, fb = NC.om_pitches(c)
    offset, mask = nans(c.B, 2 * c.third, c.P), nans(c.B, c.third, c.P)
    ok(_lib().cdfo_mv_offset_mask(vp(o1), vp(o2), ld, vp(flow), fb, c.B, c.P, c.third, NC.OM_MAG, vp(offset), vp(mask), _stream()))
    return offset, mask


def _om_bwd(c, o1, o2, goff, gmask):
    ld, _ = NC.om_pitches(c)
    g1, g2 = nans(c.B, c.P, ld), nans(c.B, c.P, ld)
    ok(_lib().cdfo_mv_offset_mask_bwd(vp(o1), vp(o2), ld, vp(goff), vp(gmask), c.B, c.P, c.third, NC.OM_MAG, vp(g1), vp(g2), _stream()))
    return g1, g2


@pytest.mark.parametrize("c", NC.OM_CASES, ids=NC.case_id)
def test_mv_offset_mask(c):
    o1, o2, flow, _, _ = (dev(t) for t in NC.om_inputs(c))
    offset, mask = _om(c, o1, o2, flow)
    ref, ref32 = NC.om_ref(c), NC.om_ref(c, torch.float32)
    _within(f"mv_offset_mask {NC.case_id(c)} offset", offset, ref[0], ref32[0])
    _within(f"mv_offset_mask {NC.case_id(c)} mask", mask, ref[1], ref32[1])


@pytest.mark.parametrize("c", NC.OM_CASES, ids=NC.case_id)
def test_mv_offset_mask_bwd(c):
    o1, o2, _, goff, gmask = (dev(t) for t in NC.om_inputs(c))
    g1, g2 = _om_bwd(c, o1, o2, goff, gmask)
    n = 3 * c.third
    ref, ref32 = NC.om_grad_ref(c), NC.om_grad_ref(c, torch.float32)
    _within(f"mv_offset_mask_bwd {NC.case_id(c)} g1", g1[..., :n], ref[0], ref32[0])
    _within(f"mv_offset_mask_bwd {NC.case_id(c)} g2", g2[..., :n], ref[1], ref32[1])
    assert g1[..., n:].isnan().all() and g2[..., n:].isnan().all()          # the padding of a pitched output is not touched
    for a, b in zip((g1, g2), _om_bwd(c, o1, o2, goff, gmask)):
        assert torch.equal(_bits(a), _bits(b))


def test_offset_mask_autograd():
    from cdfo_amd import nchw_autograd as A
    c = NC.OmCase(2, 65, 18, False)
    o1, o2, flow, goff, gmask = NC.om_inputs(c)
    H, W = 5, 13
    h1, h2 = (t.view(c.B, H, W, 3 * c.third).cuda().requires_grad_() for t in (o1, o2))
    offset, mask = A.offset_mask(h1, h2, flow.view(c.B, 2, H, W).cuda(), c.third, NC.OM_MAG)
    assert tuple(offset.shape) == (c.B, 2 * c.third, H, W) and tuple(mask.shape) == (c.B, c.third, H, W)
    torch.autograd.backward((offset, mask), (goff.view(offset.shape).cuda(), gmask.view(mask.shape).cuda()))
    ref, ref32 = NC.om_ref(c), NC.om_ref(c, torch.float32)
    _within("autograd offset", offset.detach().view(ref[0].shape), ref[0], ref32[0])
    _within("autograd mask", mask.detach().view(ref[1].shape), ref[1], ref32[1])
    gref, gref32 = NC.om_grad_ref(c), NC.om_grad_ref(c, torch.float32)
    _within("autograd offset_mask g1", h1.grad.view(gref[0].shape), gref[0], gref32[0])
    _within("autograd offset_mask g2", h2.grad.view(gref[1].shape), gref[1], gref32[1])


# ------------------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("H,W", NC.LAYOUT_P)
@pytest.mark.parametrize("Cc", NC.LAYOUT_C)
def test_layout_transposes(Cc, H, W):
    """cdfo_nchw_to_nhwc / cdfo_nhwc_to_nchw: bit-exact against permute, pitched sides (ldo, ldi > C) with their NaN padding
    untouched, both round trips; then the wrappers the autograd layout Functions run on."""
    from cdfo_amd import kernels as K
    from cdfo_amd import nchw_autograd as A
    B = NC.LAYOUT_B
    x = NC.layout_input(Cc, H, W)
    want = torch.empty(B, H, W, Cc).copy_(x.permute(0, 2, 3, 1))          # dense strides at extents of 1 too
    xd = x.cuda()
    for ld in (Cc, Cc + 3):
        pm = nans(B, H, W, ld)
        ok(_lib().cdfo_nchw_to_nhwc(vp(xd), vp(pm), B, Cc, H, W, ld, _stream()))
        assert torch.equal(pm[..., :Cc].cpu(), want) and pm[..., Cc:].isnan().all()
        back = nans(B, Cc, H, W)
        ok(_lib().cdfo_nhwc_to_nchw(vp(pm), ld, vp(back), B, Cc, H, W, _stream()))
        assert torch.equal(back.cpu(), x)
        # the other round trip: pixel-major -> NCHW -> pixel-major
        src = nans(B, H, W, ld)
        src[..., :Cc] = want.cuda()
        mid = nans(B, Cc, H, W)
        ok(_lib().cdfo_nhwc_to_nchw(vp(src), ld, vp(mid), B, Cc, H, W, _stream()))
        assert torch.equal(mid.cpu(), x)
        again = nans(B, H, W, ld)
        ok(_lib().cdfo_nchw_to_nhwc(vp(mid), vp(again), B, Cc, H, W, ld, _stream()))
        assert torch.equal(again[..., :Cc].cpu(), want) and again[..., Cc:].isnan().all()
    assert torch.equal(K.nchw_to_nhwc(xd).cpu(), want) and torch.equal(K.nhwc_to_nchw(want.cuda()).cpu(), x)
    leaf = xd.clone().requires_grad_()
    y = A.to_nchw(A.to_pixel_major(leaf))
    y.backward(xd)
    assert torch.equal(y.detach().cpu(), x) and torch.equal(leaf.grad.cpu(), x)


# ------------------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_return_einval_without_a_launch():
    """Every argument check of the fourteen entry points, once.  The output buffer stays NaN: nothing was launched."""
    L = _lib()
    s = _stream()
    t = nans(64)
    out = nans(64)
    idx = torch.zeros(64, dtype=torch.int32, device="cuda")
    p, o, i = vp(t), vp(out), vp(idx)
    conv = lambda B=1, Cc=1, H=4, W=4, Co=1, kh=3, kw=3, st=1, pad=0: L.cdfo_conv2d_nchw(p, p, p, B, Cc, H, W, Co, kh, kw, st, pad, 0, o, s)   # noqa: E731
    convb = lambda B=1, Cc=1, H=4, W=4, Co=1, kh=3, kw=3, st=1, pad=0, x=p, w=p, g=p, gin=o, gw=o, gb=o: L.cdfo_conv2d_nchw_bwd(  # noqa: E731
        x, w, g, B, Cc, H, W, Co, kh, kw, st, pad, gin, gw, gb, s)
    pool = lambda BC=1, H=4, W=4, k=2, st=2: L.cdfo_maxpool_nchw(p, BC, H, W, k, st, o, s)                 # noqa: E731
    poolb = lambda BC=1, H=4, W=4, k=2, st=2, ix=i: L.cdfo_maxpool_nchw_bwd(p, p, BC, H, W, k, st, ix, o, s)   # noqa: E731
    rs = lambda BC=1, H=2, W=2, Ho=4, Wo=4: L.cdfo_resize_bilinear_nchw(p, BC, H, W, Ho, Wo, 0, o, s)      # noqa: E731
    rsb = lambda BC=1, H=2, W=2, Ho=4, Wo=4: L.cdfo_resize_bilinear_nchw_bwd(p, BC, H, W, Ho, Wo, o, s)    # noqa: E731
    ew = lambda n=16, P=4, mode=0, a=p, b=p, x=p, y=p: L.cdfo_ew_nchw(a, b, x, y, n, P, mode, o, s)        # noqa: E731
    ewb = lambda n=16, P=4, mode=1, g=p, y=p, a=p, x=p, yv=p, out=o: L.cdfo_ew_nchw_bwd(g, y, a, x, yv, n, P, mode, out, s)   # noqa: E731
    om = lambda B=1, P=4, third=1, ld=3: L.cdfo_mv_offset_mask(p, p, ld, p, 2 * P, B, P, third, 1.0, o, o, s)   # noqa: E731
    omb = lambda B=1, P=4, third=1, ld=3: L.cdfo_mv_offset_mask_bwd(p, p, ld, p, p, B, P, third, 1.0, o, o, s)  # noqa: E731
    calls = {
        "conv B": conv(B=0), "conv C": conv(Cc=0), "conv Co": conv(Co=0), "conv kh": conv(kh=0), "conv kw": conv(kw=0),
        "conv stride": conv(st=0), "conv pad": conv(pad=-1), "conv Ho": conv(H=2), "conv Wo": conv(W=2),
        "conv Ho, C's division": conv(H=2, st=2), "conv_bwd B": convb(B=0), "conv_bwd C": convb(Cc=0), "conv_bwd Co": convb(Co=0),
        "conv_bwd kh": convb(kh=0), "conv_bwd kw": convb(kw=0), "conv_bwd stride": convb(st=0), "conv_bwd pad": convb(pad=-1),
        "conv_bwd gout": convb(g=None), "conv_bwd Ho": convb(H=2), "conv_bwd Wo": convb(W=2, st=2),
        "conv_bwd gin without w": convb(w=None), "conv_bwd gw without in": convb(x=None),
        "pool BC": pool(BC=0), "pool k": pool(k=0), "pool stride": pool(st=0), "pool H < k": pool(H=1), "pool W < k": pool(W=1),
        "pool H < k, C's division": pool(H=6, W=8, k=7, st=3),
        "pool_bwd BC": poolb(BC=0), "pool_bwd k": poolb(k=0), "pool_bwd stride": poolb(st=0), "pool_bwd H < k": poolb(H=1),
        "pool_bwd W < k, C's division": poolb(H=8, W=6, k=7, st=3), "pool_bwd scratch": poolb(ix=None),
        "pool_bwd plane of 2^31": poolb(H=65536, W=32768),
        "resize BC": rs(BC=0), "resize H": rs(H=0), "resize W": rs(W=0), "resize Ho": rs(Ho=0), "resize Wo": rs(Wo=0),
        "resize_bwd BC": rsb(BC=0), "resize_bwd H": rsb(H=0), "resize_bwd W": rsb(W=0), "resize_bwd Ho": rsb(Ho=0),
        "resize_bwd Wo": rsb(Wo=0),
        "avgpool BC": L.cdfo_avgpool_nchw(p, 0, 4, o, s), "avgpool P": L.cdfo_avgpool_nchw(p, 1, 0, o, s),
        "ew n": ew(n=0), "ew mode -1": ew(mode=-1), "ew mode 4": ew(mode=4), "ew mode 0 without b": ew(b=None),
        "ew mode 3 without x": ew(mode=3, x=None), "ew mode 3 without y": ew(mode=3, y=None), "ew mode 3 P": ew(mode=3, P=0),
        "ew_bwd n": ewb(n=0), "ew_bwd g": ewb(g=None), "ew_bwd out": ewb(out=None), "ew_bwd mode 1 without y": ewb(y=None),
        "ew_bwd mode 2 without y": ewb(mode=2, y=None), "ew_bwd mode 4 P": ewb(mode=4, P=0),
        "ew_bwd mode 5 without a": ewb(mode=5, a=None), "ew_bwd mode 5 without yv": ewb(mode=5, yv=None),
        "ew_bwd mode 5 without x": ewb(mode=5, x=None), "ew_bwd mode 5 P": ewb(mode=5, P=0),
        "ew_bwd mode 6 without a": ewb(mode=6, a=None), "ew_bwd mode 0": ewb(mode=0), "ew_bwd mode 3": ewb(mode=3),
        "ew_bwd mode 7": ewb(mode=7),
        "gate_y BC": L.cdfo_gate_nchw_bwd_y(p, p, p, 0, 4, o, s), "gate_y P": L.cdfo_gate_nchw_bwd_y(p, p, p, 1, 0, o, s),
        "om B": om(B=0), "om P": om(P=0), "om third": om(third=0), "om ld < 3 third": om(ld=2),
        "om 2^32 workgroups": om(B=65536, P=64 * 65536),
        "om_bwd B": omb(B=0), "om_bwd P": omb(P=0), "om_bwd third": omb(third=0), "om_bwd ld < 3 third": omb(ld=2),
        "om_bwd 2^32 workgroups": omb(B=65536, P=64 * 65536),
        "to_nhwc B": L.cdfo_nchw_to_nhwc(p, o, 0, 2, 2, 2, 2, s), "to_nhwc C": L.cdfo_nchw_to_nhwc(p, o, 1, 0, 2, 2, 2, s),
        "to_nhwc H": L.cdfo_nchw_to_nhwc(p, o, 1, 2, 0, 2, 2, s), "to_nhwc W": L.cdfo_nchw_to_nhwc(p, o, 1, 2, 2, 0, 2, s),
        "to_nhwc ldo < C": L.cdfo_nchw_to_nhwc(p, o, 1, 2, 2, 2, 1, s),
        "to_nchw B": L.cdfo_nhwc_to_nchw(p, 2, o, 0, 2, 2, 2, s), "to_nchw C": L.cdfo_nhwc_to_nchw(p, 2, o, 1, 0, 2, 2, s),
        "to_nchw H": L.cdfo_nhwc_to_nchw(p, 2, o, 1, 2, 0, 2, s), "to_nchw W": L.cdfo_nhwc_to_nchw(p, 2, o, 1, 2, 2, 0, s),
        "to_nchw ldi < C": L.cdfo_nhwc_to_nchw(p, 1, o, 1, 2, 2, 2, s),
    }
    wrong = {k: v for k, v in calls.items() if v != EINVAL}
    assert not wrong, wrong
    torch.cuda.synchronize()
    assert out.isnan().all() and (idx == 0).all()
    from cdfo_amd import nchw as N
    from cdfo_amd._lib import CdfoError
    with pytest.raises(CdfoError):
        N.maxpool(torch.zeros(1, 1, 6, 8, device="cuda"), 7, 3)
