"""LPIPS as a training loss without a device: the float statement (tests/lpips_loss_ref.py) is tied to the metric's statement and to
central differences; the closed forms the adjoint kernels of csrc/lpips.hip compute -- the distance's derivative, the pool's routing
rule, the stem's folded weights -- are restated in numpy and held against torch's autograd; the committed cases of the device test
satisfy the kink condition; and every refusal that needs no device is reached."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_cases as metric_cases
import lpips_loss_cases as cases
import lpips_loss_ref as ref
import lpips_ref


# ---- the statement ----
@pytest.mark.parametrize("normalize", [True, False])
def test_float_statement_on_k_over_255_has_the_bits_of_the_metric(normalize):
    """x = fp32(k) / 255 through an fp32 trunk: the bits of `lpips_ref.layers` on the uint8 frame k."""
    params = metric_cases.model(metric_cases.NARROW, 11)
    sr, gt = metric_cases.frames((17, 19), (17, 19), 2, 5)
    for a, b in zip(sr, gt):
        xa, xb = torch.from_numpy(a).to(torch.float32) / 255, torch.from_numpy(b).to(torch.float32) / 255
        got = ref.layers(xa, xb, params, normalize, trunk_dtype=torch.float32).numpy()
        want = lpips_ref.layers(a, b, params, normalize, trunk_dtype=torch.float32)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
        assert float(ref.total(torch.from_numpy(got))) == lpips_ref.total(want)


def test_gradient_agrees_with_central_differences():
    """The fp64 statement's autograd gradient against (L(x + e) - L(x - e)) / 2e, e = 1e-6, at 24 pixels of a 16 x 16 frame.
    Measured: the largest difference is 8.3e-10 of the largest |gradient| (the differences' own truncation and cancellation:
    e^2 times a third derivative, and 1e-16 / e); asserted: 8 x that, 7e-9.  A missing ReLU select or a misrouted pool moves single
    pixels by a few per cent."""
    params, sr, hr, _ = cases.case("w2-16x16-n1")
    x, y = torch.tensor(sr[0], dtype=torch.float64), torch.tensor(hr[0], dtype=torch.float64)
    g = ref.gradient(sr[:1], hr[:1], params, (1.0,))[0]
    rs, e, worst = np.random.RandomState(0), 1e-6, 0.0
    f = lambda t: float(ref.total(ref.layers(t, y, params)))
    for i, j in zip(rs.randint(0, 16, 24), rs.randint(0, 16, 24)):
        d = torch.zeros_like(x)
        d[i, j] = e
        worst = max(worst, abs((f(x + d) - f(x - d)) / (2 * e) - g[i, j]))
    gap = worst / np.abs(g).max()
    print(f"central differences: {gap:.3g} of max |g|")
    assert gap < 7e-9


# ---- (b) the distance's derivative ----
def np_dist_bwd(fa, fb, lin, gscale, gin=None):
    """The closed form of cdfo_lpips_dist_bwd in numpy fp64: fa, fb [N,h,w,C], lin [C], gscale [N], gin [N,h,w,C] or None."""
    A, B = fa.astype(np.float64), fb.astype(np.float64)
    N, h, w, _ = A.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        na = np.sqrt((A * A).sum(axis=3, keepdims=True))
        r, rb = 1 / (na + 1e-10), 1 / (np.sqrt((B * B).sum(axis=3, keepdims=True)) + 1e-10)
        u = A * r - B * rb
        q = (lin * u * A).sum(axis=3, keepdims=True)
        t = np.asarray(gscale, dtype=np.float64)[:, None, None, None] / (h * w) * 2 * r * (lin * u - (r * q / na) * A)
        if gin is not None:
            t = t + gin
    return np.where(A > 0, t, 0.0)


@pytest.mark.parametrize("C", [16, 48, 80])
@pytest.mark.parametrize("with_gin", [False, True])
def test_closed_form_of_the_distance_gradient_equals_autograd(C, with_gin):
    pre, fa, fb, lin, gscale, gin = cases.dist_case(C, 3, 5)
    gin = gin if with_gin else None
    assert float(lpips_ref.layer_distance(torch.from_numpy(fa[0]).permute(2, 0, 1), torch.from_numpy(fb[0]).permute(2, 0, 1), lin)) == \
        float(ref.layer_distance(torch.from_numpy(fa[0]).permute(2, 0, 1), torch.from_numpy(fb[0]).permute(2, 0, 1), lin))
    got, want = np_dist_bwd(fa, fb, lin, gscale, gin), cases.dist_bwd_autograd(pre, fb, lin, gscale, gin)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    assert not got[0, 0, 0].any() and not want[0, 0, 0].any()             # the all-zero pixel: 0 / 0 dropped by the select
    if not with_gin:
        assert not got[1].any() and not want[1].any()                     # the frame with gscale 0
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


# ---- (c) the pool's routing ----
def np_pool2_bwd(x, g):
    """x [N,H,W,C], g [N,H//2,W//2,C] -> gx [N,H,W,C]: the routing rule of cdfo_lpips_pool2_bwd."""
    N, H, W, C = x.shape
    gx = np.zeros_like(x)
    for y in range(H // 2):
        for xx in range(W // 2):
            win = [x[:, 2 * y + dy, 2 * xx + dx] for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))]
            m, k = win[0].copy(), np.zeros((N, C), dtype=np.int64)
            for i in (1, 2, 3):
                with np.errstate(invalid="ignore"):
                    take = (win[i] > m) | np.isnan(win[i])
                m, k = np.where(take, win[i], m), np.where(take, i, k)
            for i, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                gx[:, 2 * y + dy, 2 * xx + dx] = np.where(k == i, g[:, y, xx], 0.0)
    return gx


@pytest.mark.parametrize("size", [(2, 2), (3, 3), (5, 8), (17, 19)])
def test_routing_rule_equals_max_pool2d_backward(size):
    x, g = cases.pool_case(*size, 4)
    got, want = np_pool2_bwd(x, g), cases.torch_pool2_bwd(x, g)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not got[:, size[0] // 2 * 2:].any() and not got[:, :, size[1] // 2 * 2:].any()


# ---- (d) the stem's folded weights ----
@pytest.mark.parametrize("normalize", [True, False])
def test_folded_stem_weights_are_the_adjoint_of_scaling_and_conv1_1(normalize):
    from cdfo_amd import metrics as M
    params = cases.model(cases.W1, 21)
    wf = M.lpips_stem_adjoint(params.weights[0], normalize)
    assert wf.dtype == np.float32 and wf.shape == (16, 3, 3)
    rs = np.random.RandomState(3)
    g = torch.from_numpy(rs.randn(1, 16, 7, 9))
    x = torch.zeros(7, 9, dtype=torch.float64, requires_grad=True)
    w0 = torch.from_numpy(np.array(params.weights[0])).to(torch.float64)
    (F.conv2d(ref.trunk_input(x, normalize), w0, padding=1) * g).sum().backward()
    folded = F.conv2d(g, torch.from_numpy(wf).to(torch.float64).flip(1, 2)[None], padding=1)[0, 0]
    assert float((folded - x.grad).abs().max()) <= 4e-7 * float(x.grad.abs().max())      # wf is rounded to fp32 once: 2^-24 per weight


# ---- the kink condition of the device test's cases ----
@pytest.mark.parametrize("name", list(cases.CASES))
def test_committed_cases_keep_clear_of_the_kinks(name):
    """A condition on the inputs, not a measurement: the result's frames sit at least 8 x the fp32 trunk's drift away from every
    ReLU's zero and every live pool window's tie, so the fp32 device and the fp64 statement differentiate the same branch."""
    params, sr, _, _ = cases.case(name)
    relu, pool, drift = ref.kinks(sr, params)
    print(f"{name}: min |pre| {relu:.3g}, min pool gap {pool:.3g}, fp32 drift {drift:.3g}, ratio {min(relu, pool) / drift:.1f}")
    assert min(relu, pool) >= 8 * drift


# ---- refusals that need no device ----
def test_refusals_before_any_device_work(monkeypatch):
    from cdfo_amd import _lib, kernels as K, metrics as M
    from cdfo_amd.loss import lpips_loss
    from cdfo_amd.train import fit
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was looked up"))
    params = cases.model(cases.W1, 21)
    x = torch.zeros(2, 1, 16, 16)
    for bad in (lambda: lpips_loss(x, x, params), lambda: lpips_loss(x, x, {"w0": 1}), lambda: M.lpips_layers_f32(x, x, params),
                lambda: K.lpips_stem_f32(x[:, 0], torch.zeros(16, 3, 3, 3), torch.zeros(16)),
                lambda: K.lpips_dist_bwd(x, x, torch.zeros(16, dtype=torch.float64), torch.zeros(2)),
                lambda: K.lpips_pool2_bwd(x, x), lambda: K.lpips_stem_bwd(x, torch.zeros(16, 3, 3))):
        with pytest.raises(ValueError):
            bad()
    model = torch.nn.Linear(1, 1)
    for kw in (dict(lpips=params), dict(lpips=params, lpips_weight=0.0), dict(lpips=params, lpips_weight=-1.0),
               dict(lpips=params, lpips_weight=float("nan")), dict(lpips=params, lpips_weight=float("inf")),
               dict(lpips_weight=0.5), dict(lpips=params, lpips_weight=0.5, crop=3), dict(lpips={"w0": 1}, lpips_weight=0.5)):
        with pytest.raises(ValueError, match="lpips|LPIPS"):
            fit(model, None, 1, "/nonexistent/out", **kw)
