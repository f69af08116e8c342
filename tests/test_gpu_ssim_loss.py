"""`cdfo_amd.loss.ssim_loss` and `msssim_loss` on the device against the fp64 statement (tests/ssim_loss_ref.py) on every case of
tests/ssim_loss_cases.py with a non-unit upstream gradient per frame, within the derived bounds of that file; their identities; the
evaluators' SSIM and MS-SSIM within the loss bound; every promised error.

Worst measured / bound on the MI355X over the 36 cases (each test prints its own): the loss 0.469 (L1-64x64-n1-s0.5), the gradient
0.452 (L5-176x176-n2-s0.05); identical frames: loss exactly 0, max |g| 2e-18; against metrics.calculate_ssim 0.055 and against
metrics.msssim_u8 0.194 of the loss bound.  No derived bound was missed."""
import numpy as np
import pytest
import torch

import msssim_ref
import ssim_loss_cases as cases

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _fn(levels):
    from cdfo_amd.loss import msssim_loss, ssim_loss
    return ssim_loss if levels == 1 else msssim_loss


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize("c", cases.CASES + (cases.CLAMP,), ids=cases.case_id)
def test_loss_and_gradient_match_the_fp64_statement(c):
    levels, _, _, n, _, peak = c
    f = _fn(levels)
    sr, hr = cases.case(c)
    l64, g64, _, _ = cases.reference(c)
    up = _dev(cases.upstream(n))
    x, y = _dev(sr)[:, None].requires_grad_(True), _dev(hr)[:, None].requires_grad_(True)
    loss = f(x, y, peak)
    assert loss.dtype == torch.float32 and loss.shape == (n,) and loss.requires_grad
    loss.backward(gradient=up)
    assert y.grad is None and x.grad.shape == x.shape and x.grad.dtype == torch.float32
    rl, rg = cases.loss_ratio(loss.detach().cpu().numpy(), l64), cases.grad_ratio(x.grad[:, 0].cpu().numpy(), g64)
    print("%s: measured / bound: loss %.3f, gradient %.3f" % (cases.case_id(c), rl, rg))
    assert rl <= 1 and rg <= 1
    if n == 3:                                                               # upstream 0: zeros
        assert not x.grad[1].any() and x.grad[0].any()
    if c == cases.CLAMP:
        assert (loss.detach().cpu().numpy() == 1.0).all() and not x.grad.any()
    # the three-dimensional form and a second run: equal bits, forward and backward
    x3 = _dev(sr).requires_grad_(True)
    loss3 = f(x3, _dev(hr), peak)
    loss3.backward(gradient=up)
    assert torch.equal(_bits(loss3), _bits(loss)) and torch.equal(_bits(x3.grad), _bits(x.grad[:, 0]))


@pytest.mark.parametrize("c", (cases.SSIM_CASES[-2], cases.SSIM_CASES[-1], cases.MS_CASES[2]), ids=cases.case_id)
def test_identical_frames(c):
    levels, _, _, n, _, peak = c
    _, hr = cases.case(c)
    x = _dev(hr).requires_grad_(True)
    loss = _fn(levels)(x, _dev(hr), peak)
    loss.sum().backward()
    el, eg = float(loss.detach().abs().max()), float(x.grad.abs().max())
    print("%s, sr == hr: |loss| %.2g (bound 1e-9), max |g| %.2g (bound %.2g)" % (cases.case_id(c), el, eg, 1e-9 / peak))
    assert el <= 1e-9 and eg <= 1e-9 / peak


def test_ssim_loss_is_one_minus_the_evaluators_ssim():
    from cdfo_amd import metrics
    from cdfo_amd.loss import ssim_loss
    c = cases.SSIM_CASES[-1]                                                  # peak 255 on frames times 255
    sr, hr = (_dev(a) for a in cases.case(c))
    want = 1.0 - metrics.calculate_ssim(sr, hr, crop_border=0, from_unit_range=False).cpu().numpy()
    r = cases.loss_ratio(ssim_loss(sr, hr, 255.0).cpu().numpy(), want)
    print("1 - ssim_loss(peak 255) against metrics.calculate_ssim: measured / bound %.3f" % r)
    assert r <= 1


def test_msssim_loss_is_one_minus_the_evaluators_msssim():
    """8-bit-valued float frames: pooled integers are exact in fp32 up to level 4, so the fp32 pyramid costs nothing."""
    from cdfo_amd import metrics
    from cdfo_amd.loss import msssim_loss
    a, b = msssim_ref.correlated_pair(3, (177, 191), 255, 12.0, seed=3)
    want = 1.0 - metrics.msssim_u8(_dev(b), _dev(a), crop_border=0).cpu().numpy()
    got = msssim_loss(_dev(b.astype(np.float32)), _dev(a.astype(np.float32)), 255.0).cpu().numpy()
    r = cases.loss_ratio(got, want)
    print("msssim_loss(peak 255) against 1 - metrics.msssim_u8: measured / bound %.3f" % r)
    assert r <= 1 and abs(got[1]) <= 1e-9                                     # frame 1 of the pair is identical


def test_no_grad_skips_the_gradient_passes(monkeypatch):
    """Asserted by what the wrapper returns: no gradient tensor exists when none is wanted."""
    from cdfo_amd import kernels as K
    from cdfo_amd.loss import msssim_loss, ssim_loss
    sr, hr = (_dev(a) for a in cases.case(cases.MS_CASES[0]))
    seen, inner = [], K.ssim_loss

    def spy(*a, **kw):
        out = inner(*a, **kw)
        seen.append(out[1])
        return out

    for f in (ssim_loss, msssim_loss):
        monkeypatch.setattr(K, "ssim_loss", spy)
        del seen[:]
        plain = f(sr, hr)                                                    # no input needs a gradient
        with torch.no_grad():
            quiet = f(sr.clone().requires_grad_(True), hr)
        only_hr = f(sr, hr.clone().requires_grad_(True))
        assert seen == [None, None, None]
        assert not plain.requires_grad and not quiet.requires_grad and not only_hr.requires_grad
        monkeypatch.undo()
        loud = f(sr.clone().requires_grad_(True), hr)
        assert loud.requires_grad and torch.equal(loud.detach(), plain) and torch.equal(quiet, plain) and torch.equal(only_hr, plain)


def test_every_promised_error():
    from cdfo_amd.loss import msssim_loss, ssim_loss
    sr, hr = (_dev(a) for a in cases.case(cases.MS_CASES[0]))                  # [2,176,176]
    wide = torch.zeros((2, 176, 352), device="cuda")
    z = lambda *s: torch.zeros(s, device="cuda")                                               # noqa: E731
    for f in (ssim_loss, msssim_loss):
        for bad in (lambda: f(sr.double(), hr), lambda: f(sr, hr.half()), lambda: f(wide[:, :, :176], hr),
                    lambda: f(sr.transpose(1, 2), hr.transpose(1, 2)), lambda: f(sr, hr[:1]),
                    lambda: f(sr[:, None].expand(2, 3, 176, 176), hr[:, None].expand(2, 3, 176, 176)), lambda: f(z(176, 176), z(176, 176)),
                    lambda: f(z(0, 176, 176), z(0, 176, 176)), lambda: f(z(1, 10, 200), z(1, 10, 200)), lambda: f(z(1, 200, 10), z(1, 200, 10)),
                    lambda: f(sr, hr, 0.0), lambda: f(sr, hr, -1.0), lambda: f(sr, hr, float("nan")), lambda: f(sr, hr, float("inf")),
                    lambda: f(sr, hr, True), lambda: f(sr, hr, "1")):
            with pytest.raises(ValueError):
                bad()
        with pytest.raises(NotImplementedError):
            f(sr.cpu(), hr.cpu())
        with pytest.raises(NotImplementedError):
            f(sr, hr.cpu())
    for bad in (lambda: msssim_loss(z(1, 175, 200), z(1, 175, 200)), lambda: msssim_loss(z(1, 200, 175), z(1, 200, 175))):
        with pytest.raises(ValueError):
            bad()
    assert ssim_loss(z(1, 11, 175), z(1, 11, 175)).shape == (1,)             # fine for one scale
