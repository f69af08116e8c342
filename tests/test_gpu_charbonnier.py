"""The Charbonnier loss on the device (csrc/train_batch.hip: cdfo_charbonnier; cdfo_amd/loss.py) against the float64 statement
``sum(sqrt((sr - hr)^2 + eps))`` evaluated on the fp32 inputs.

Tolerances, from the arithmetic.  A term takes one fp32 rounding each for d, d^2, + eps and the square root; the square root halves
what went in, so a term is within 1.8e-7 of the truth, relatively.  All terms are positive: the sum inherits the bound.  The fp64
accumulation is negligible, the final rounding to fp32 adds 6e-8.  rtol 5e-7 leaves a factor of 2.  The gradient d / sqrt(d^2 + eps)
sees three roundings beyond d's own, <= 3e-7: rtol 1e-6 leaves a factor of 3."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
EPS = 1e-4
SHAPES = [(1,), (255,), (256 * 5 + 3,), (2, 1, 32, 32), (3, 1, 48, 80)]


def inputs(shape, seed):
    """fp32 pairs with |d| up to 1, entries with d = 0 exactly and (where there is room) d = 1 and d = -1."""
    rs = np.random.RandomState(seed)
    hr = rs.rand(*shape).astype(np.float32)
    sr = rs.rand(*shape).astype(np.float32)
    n = hr.size
    sr.reshape(-1)[::5] = hr.reshape(-1)[::5]
    if n > 4:
        hr.reshape(-1)[1], sr.reshape(-1)[1] = 0.0, 1.0
        hr.reshape(-1)[2], sr.reshape(-1)[2] = 1.0, 0.0
    return sr, hr


def statement(sr, hr):
    d = sr.astype(np.float64) - hr.astype(np.float64)
    t = np.sqrt(d * d + EPS)
    return t.sum(), d / t


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_and_gradient_against_float64(shape):
    from cdfo_amd.loss import charbonnier
    sr_np, hr_np = inputs(shape, len(shape) + shape[-1])
    sr = torch.from_numpy(sr_np).cuda().requires_grad_(True)
    hr = torch.from_numpy(hr_np).cuda()
    loss = charbonnier(sr, hr, EPS)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    want, want_g = statement(sr_np, hr_np)
    got = loss.item()
    print(f"{shape}: loss {got!r} against {want!r}, relative {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 5e-7 * want
    up = torch.tensor(-2.5, device="cuda")                       # a non-unit upstream gradient
    (g,) = torch.autograd.grad(loss, sr, grad_outputs=up)
    g = g.cpu().numpy().astype(np.float64)
    zero = sr_np == hr_np
    assert zero.any() and not g[zero].any()                      # d = 0: the term is sqrt(eps), the gradient exactly 0
    err = np.abs(g - (-2.5) * want_g)
    print(f"{shape}: gradient worst relative {np.max(err[~zero] / np.abs(2.5 * want_g[~zero]), initial=0.0):.2e}")
    assert (err <= 1e-6 * np.abs(2.5 * want_g)).all()
    assert g.shape == sr_np.shape


def test_backward_through_a_graph_and_no_gradient_for_hr():
    from cdfo_amd.loss import charbonnier
    sr_np, hr_np = inputs((2, 1, 32, 32), 3)
    w = torch.tensor(0.5, device="cuda", requires_grad=True)
    hr = torch.from_numpy(hr_np).cuda().requires_grad_(True)
    loss = charbonnier(torch.from_numpy(sr_np).cuda() * w, hr, EPS) * 3.0
    loss.backward()
    _, g = statement(sr_np * np.float32(0.5), hr_np)
    want = 3.0 * (g * sr_np.astype(np.float64)).sum()
    # behind the kernel's gradient (1e-6) torch multiplies and adds 2048 products in fp32: a tree sum with a short serial run per
    # thread, at most some 32 roundings of 6e-8 on any path, 3e-6 of the sum of magnitudes in all; 1e-5 leaves a factor of 3
    assert abs(float(w.grad) - want) <= 1e-5 * np.abs(g * sr_np).sum() * 3.0
    assert hr.grad is None


def test_two_runs_give_identical_bits():
    from cdfo_amd.loss import charbonnier
    sr_np, hr_np = inputs((3, 1, 48, 80), 9)
    sr, hr = torch.from_numpy(sr_np).cuda().requires_grad_(True), torch.from_numpy(hr_np).cuda()
    runs = []
    for _ in range(2):
        loss = charbonnier(sr, hr, EPS)
        (g,) = torch.autograd.grad(loss, sr)
        runs.append((loss.detach().cpu().numpy().view(np.uint32).item(), g.cpu().numpy().view(np.uint32)))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])


def test_non_finite_inputs_propagate():
    from cdfo_amd.loss import charbonnier
    sr_np, hr_np = inputs((256 * 5 + 3,), 4)
    sr_np[700] = np.nan
    assert np.isnan(float(charbonnier(torch.from_numpy(sr_np).cuda(), torch.from_numpy(hr_np).cuda())))
    sr_np[700] = np.inf
    assert float(charbonnier(torch.from_numpy(sr_np).cuda(), torch.from_numpy(hr_np).cuda())) == np.inf


def test_anything_but_dense_fp32_of_one_shape_is_refused():
    from cdfo_amd.loss import charbonnier
    a = torch.rand(2, 1, 32, 32, device="cuda")
    with pytest.raises(ValueError):
        charbonnier(a, torch.rand(2, 1, 32, 31, device="cuda"))
    with pytest.raises(ValueError):
        charbonnier(a, a[0])
    with pytest.raises(ValueError):
        charbonnier(a.transpose(2, 3), a)                         # equal shapes, not dense
    with pytest.raises(ValueError):
        charbonnier(a[:, :, ::2], a[:, :, ::2])
    with pytest.raises(ValueError):
        charbonnier(a.double(), a.double())
    with pytest.raises(NotImplementedError):
        charbonnier(a.cpu(), a.cpu())
