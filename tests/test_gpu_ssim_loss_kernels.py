"""The kernels of the SSIM / MS-SSIM losses (csrc/ssim_loss.hip) one entry point at a time through the C ABI, on NaN-prefilled
outputs, against the fp64 statement of tests/ssim_loss_ref.py on the cases of tests/ssim_loss_cases.py.  The pool must give the
defined rounding bit for bit; the means are held to 1e-10 (the fp64 error budget of ssim_loss_cases), the coefficients to 1e-12 of
the frame's largest, the loss and the gradient to the derived bounds; the adjoint entry point, linear in its maps and in the coarser
gradient, is put to the dot test against the statement's window and the project's own pool; every backward runs twice for equal bits.

Worst on the MI355X over the 36 cases (each test prints its own): the means 5.8e-14 from the statement's, the coefficients 2.2e-14 of
the largest (both L5-200x233-n2-s0.05), the loss 0.469 of its bound (L1-64x64-n1-s0.5), the gradient 0.247 of its bound
(L5-177x191-n2-s0.5); the dot test 2.8e-14 apart at level 1 (bound 2.8e-8).  No derived bound was missed."""
import numpy as np
import pytest
import torch

import ssim_loss_cases as cases
import ssim_loss_ref as ref

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _lib():
    from cdfo_amd import _lib as L
    return L.lib(), L._vp


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _nan(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def forward(sr, hr, peak, levels):
    """(xs, ys: the pyramid's device stacks, means [N,levels,2], coef [N,levels,2], loss [N]) through pool, level and combine."""
    lib, vp = _lib()
    N, H, W = sr.shape
    T = lib.cdfo_ssim_loss_tiles(H, W, levels)
    assert T > 0
    partial = _nan((N, T, 2), torch.float64)
    xs, ys = [sr], [hr]
    for j in range(levels):
        if j:
            h, w = H >> (j - 1), W >> (j - 1)
            xs.append(_nan((N, h >> 1, w >> 1), torch.float32))
            ys.append(_nan((N, h >> 1, w >> 1), torch.float32))
            assert lib.cdfo_ssim_loss_pool(vp(xs[j - 1]), vp(ys[j - 1]), N, h, w, vp(xs[j]), vp(ys[j]), _stream()) == 0
        assert lib.cdfo_ssim_loss_level(vp(xs[j]), vp(ys[j]), N, H, W, levels, j, peak, vp(partial), partial.numel(), _stream()) == 0
    means, coef, loss = _nan((N, levels, 2), torch.float64), _nan((N, levels, 2), torch.float64), _nan((N,), torch.float32)
    assert lib.cdfo_ssim_loss_combine(vp(partial), partial.numel(), N, H, W, levels, vp(means), vp(coef), vp(loss), _stream()) == 0
    assert not bool(torch.isnan(partial).any())
    return xs, ys, means, coef, loss


def backward(xs, ys, coef, peak, levels):
    """g fp32 [N,H,W] through pqr and adjoint, coarsest level first."""
    lib, vp = _lib()
    N, H, W = xs[0].shape
    coarse = None
    for j in range(levels - 1, -1, -1):
        h, w = H >> j, W >> j
        pqr = _nan((N, 3, h - 10, w - 10), torch.float64)
        assert lib.cdfo_ssim_loss_pqr(vp(xs[j]), vp(ys[j]), N, H, W, levels, j, peak, vp(coef), vp(pqr), pqr.numel(), _stream()) == 0
        out = _nan((N, h, w), torch.float64 if j else torch.float32)
        assert lib.cdfo_ssim_loss_adjoint(vp(pqr), vp(xs[j]), vp(ys[j]), N, H, W, levels, j, vp(coarse), vp(out if j else None),
                                          vp(None if j else out), _stream()) == 0
        coarse = out
    return coarse


@pytest.mark.parametrize("c", cases.CASES + (cases.CLAMP,), ids=cases.case_id)
def test_entry_points_against_the_statement(c):
    levels, _, _, n, _, peak = c
    sr, hr = cases.case(c)
    l64, _, m64, c64 = cases.reference(c)
    xs, ys, means, coef, loss = forward(_dev(sr), _dev(hr), peak, levels)
    # the pool: the defined rounding, bit for bit
    a, b = sr, hr
    for j in range(1, levels):
        a, b = (np.stack([ref.pool_numpy(f) for f in s]) for s in (a, b))
        assert np.array_equal(xs[j].cpu().numpy().view(np.uint32), a.view(np.uint32))
        assert np.array_equal(ys[j].cpu().numpy().view(np.uint32), b.view(np.uint32))
    em = np.abs(means.cpu().numpy() - m64).max()
    top = np.abs(c64).reshape(n, -1).max(axis=1)
    ec = np.abs(coef.cpu().numpy() - c64).reshape(n, -1).max(axis=1)
    ec = float(np.where(top > 0, ec / np.where(top > 0, top, 1), ec).max())
    rl = cases.loss_ratio(loss.cpu().numpy(), l64)
    print("%s: means %.2g (bound 1e-10), coefficients %.2g of the largest (bound 1e-12), loss measured / bound %.3f"
          % (cases.case_id(c), em, ec, rl))
    assert em <= 1e-10 and ec <= 1e-12 and rl <= 1
    # the gradient at upstream 1, twice
    _, g64, _, _ = ref.statement(sr, hr, peak, levels)
    g = backward(xs, ys, coef, peak, levels)
    again = backward(xs, ys, coef, peak, levels)
    assert torch.equal(g.view(torch.int32), again.view(torch.int32))
    rg = cases.grad_ratio(g.cpu().numpy(), g64)
    print("%s: gradient measured / bound %.3f" % (cases.case_id(c), rg))
    assert rg <= 1
    if c == cases.CLAMP:
        assert (loss.cpu().numpy() == 1.0).all() and not coef.cpu().numpy().any() and not g.cpu().numpy().any()
    # a second forward: equal bits
    _, _, means2, coef2, loss2 = forward(_dev(sr), _dev(hr), peak, levels)
    assert torch.equal(means.view(torch.int64), means2.view(torch.int64)) and torch.equal(coef.view(torch.int64), coef2.view(torch.int64))
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32))


@pytest.mark.parametrize("level", (0, 1, 4))
def test_adjoint_dot_test(level):
    """<A(p, q, r, coarse), u> = <p, G*u> + <q, G*(2 x u)> + <r, G*(y u)> + <coarse, pool(u)>: the left side from the adjoint entry
    point, the window sums from the statement, the pool from the project's own kernel (u holds small integers, so pooling them is
    exact in fp32).  Level 1 of 177 x 191 is 88 x 95: a dropped odd column.  Level 4 has no coarser level; level 0 is rounded to fp32."""
    lib, vp = _lib()
    N, H, W, levels = 2, 177, 191, 5
    h, w = H >> level, W >> level
    rs = np.random.RandomState(5 + level)
    x, y = (rs.uniform(0, 1, (N, h, w)).astype(np.float32) for _ in range(2))
    pqr = rs.randn(N, 3, h - 10, w - 10)
    u = rs.randint(-8, 9, (N, h, w)).astype(np.float32)
    coarse = rs.randn(N, h >> 1, w >> 1) if level < 4 else None
    out = _nan((N, h, w), torch.float64 if level else torch.float32)
    dx, dy, dp, dc = _dev(x), _dev(y), _dev(pqr), None if coarse is None else _dev(coarse)
    assert lib.cdfo_ssim_loss_adjoint(vp(dp), vp(dx), vp(dy), N, H, W, levels, level, vp(dc), vp(out if level else None),
                                      vp(None if level else out), _stream()) == 0
    g = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all()
    win = torch.from_numpy(ref.gaussian_kernel_11())
    fv = lambda a: ref.filter_valid(torch.from_numpy(a), win).numpy()                         # noqa: E731
    u64, x64, y64 = u.astype(np.float64), x.astype(np.float64), y.astype(np.float64)
    terms = [pqr[:, 0] * fv(u64), pqr[:, 1] * fv(2 * x64 * u64), pqr[:, 2] * fv(y64 * u64)]
    if coarse is not None:
        du, dz = _dev(u), _dev(np.zeros_like(u))
        un, zn = _nan((N, h >> 1, w >> 1), torch.float32), _nan((N, h >> 1, w >> 1), torch.float32)
        assert lib.cdfo_ssim_loss_pool(vp(du), vp(dz), N, h, w, vp(un), vp(zn), _stream()) == 0
        assert not zn.cpu().numpy().any()
        terms.append(coarse * un.cpu().numpy().astype(np.float64))
    lhs, rhs = float((g * u64).sum()), float(sum(t.sum() for t in terms))
    scale = float(sum(np.abs(t).sum() for t in terms))
    bound = 1e-12 * scale + (0.0 if level else 2.0 ** -24 * float(np.abs(g * u64).sum()))     # level 0's elements are rounded to fp32
    print("level %d: <A m, u> = %.15g, <m, A^T u> = %.15g, apart %.3g, bound %.3g" % (level, lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound


def test_one_frame_does_not_reach_another():
    """Frame 1 of three alone gives the bits it has in the batch: sums, loss and gradient."""
    c = (1, 59, 91, 3, 0.5, 1.0)
    sr, hr = cases.case(c)
    xs, ys, means, coef, loss = forward(_dev(sr), _dev(hr), 1.0, 1)
    g = backward(xs, ys, coef, 1.0, 1)
    xs1, ys1, means1, coef1, loss1 = forward(_dev(sr[1:2]), _dev(hr[1:2]), 1.0, 1)
    g1 = backward(xs1, ys1, coef1, 1.0, 1)
    assert torch.equal(means[1:2].view(torch.int64), means1.view(torch.int64)) and torch.equal(loss[1:2].view(torch.int32), loss1.view(torch.int32))
    assert torch.equal(g[1:2].view(torch.int32), g1.view(torch.int32))
