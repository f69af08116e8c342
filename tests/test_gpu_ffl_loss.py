"""`cdfo_amd.loss.focal_frequency_loss` on the device against the fp64 statement (tests/ffl_ref.py) on every case and alpha of
tests/ffl_cases.py with a non-unit upstream gradient per frame, its identities, and `train.fit` with the term.  The bound of a
shape is 16 x the fp32 floor measured when the test runs (ffl_cases.floors).

Worst measured / bound on the MI355X over the 180 (case, alpha) pairs (each test prints its own): the loss 0.155 (16x256-patterns,
alpha 1; errors 0.3e-7 .. 3.0e-7 of the loss against floors of 1.2e-7 .. 2.5e-7), the gradient 0.132 (16x256-patterns, alpha 0;
1.4e-7 .. 8.1e-7 of max |g| against 2.8e-7 .. 4.4e-7): the device is within 2.5 x the fp32 floor everywhere."""
import re

import numpy as np
import pytest
import torch

import ffl_cases as cases

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


@pytest.mark.parametrize("alpha", cases.ALPHAS)
@pytest.mark.parametrize("c", cases.CASES, ids=cases.case_id)
def test_loss_and_gradient_match_the_fp64_statement(c, alpha):
    from cdfo_amd.loss import focal_frequency_loss
    h, w, kind = c
    sr, hr = cases.case(*c)
    _, l64, g64 = cases.reference(h, w, kind, alpha)
    _, fl, fg = cases.floors(h, w)
    x, y = _dev(sr)[:, None].requires_grad_(True), _dev(hr)[:, None].requires_grad_(True)
    loss = focal_frequency_loss(x, y, alpha)
    assert loss.dtype == torch.float32 and loss.shape == (len(l64),) and loss.requires_grad
    loss.backward(gradient=_dev(cases.upstream(len(l64))))
    assert y.grad is None and x.grad.shape == x.shape and x.grad.dtype == torch.float32
    el, eg = cases.loss_err(loss.detach().cpu().numpy(), l64).max(), cases.grad_err(x.grad[:, 0].cpu().numpy(), g64).max()
    print("%s alpha %g: loss %.3g of itself, bound %.3g, measured / bound %.3f; gradient %.3g of max |g|, bound %.3g, measured / bound "
          "%.3f" % (cases.case_id(c), alpha, el, cases.MARGIN * fl, el / (cases.MARGIN * fl), eg, cases.MARGIN * fg,
                    eg / (cases.MARGIN * fg)))
    assert el <= cases.MARGIN * fl and eg <= cases.MARGIN * fg
    # the three-dimensional form and a second run: equal bits, forward and backward
    x3 = _dev(sr).requires_grad_(True)
    loss3 = focal_frequency_loss(x3, _dev(hr), alpha)
    loss3.backward(gradient=_dev(cases.upstream(len(l64))))
    assert torch.equal(loss3.detach().view(torch.int32), loss.detach().view(torch.int32))
    assert torch.equal(x3.grad.view(torch.int32), x.grad[:, 0].view(torch.int32))


def test_identities():
    from cdfo_amd.loss import focal_frequency_loss
    sr, hr = cases.case(64, 64, "random-n3")                                    # three frames
    for alpha in cases.ALPHAS:
        # sr equal to hr in bits: exactly 0 and an all-zero gradient (the 0 / 0 weights are 0 by the NaN rule; at alpha = 0 they are 1)
        x = _dev(hr).requires_grad_(True)
        loss = focal_frequency_loss(x, _dev(hr), alpha)
        loss.sum().backward()
        assert not loss.detach().cpu().numpy().any() and not x.grad.cpu().numpy().any()
    # alpha = 0: mean(d^2), within the fp32 floor's margin, and the gradient 2 d / (H W)
    d = (sr - hr).astype(np.float64)
    x = _dev(sr).requires_grad_(True)
    loss = focal_frequency_loss(x, _dev(hr), 0.0)
    loss.sum().backward()
    _, fl, fg = cases.floors(64, 64)
    live = d.any(axis=(1, 2))
    assert cases.loss_err(loss.detach().cpu().numpy(), (d ** 2).mean(axis=(1, 2)))[live].max() <= cases.MARGIN * fl
    assert cases.grad_err(x.grad.cpu().numpy(), 2 * d / d[0].size).max() <= cases.MARGIN * fg
    # a frame with upstream gradient 0 gets zeros
    x = _dev(sr).requires_grad_(True)
    focal_frequency_loss(x, _dev(hr)).backward(gradient=torch.tensor([1.0, 0.0, 0.5], device="cuda"))
    assert x.grad[0].any() and not x.grad[1].any()
    # nothing is cast or made contiguous behind the caller's back, and sizes outside the set are refused
    a, b = _dev(sr), _dev(hr)
    wide = torch.zeros((3, 64, 128), device="cuda")
    z = lambda *s: torch.zeros(s, device="cuda")                                               # noqa: E731
    for bad in (lambda: focal_frequency_loss(a.double(), b), lambda: focal_frequency_loss(a, b.half()),
                lambda: focal_frequency_loss(wide[:, :, :64], b), lambda: focal_frequency_loss(a.transpose(1, 2), b.transpose(1, 2)),
                lambda: focal_frequency_loss(a, b[:2]), lambda: focal_frequency_loss(a[:, None].expand(3, 3, 64, 64), b[:, None].expand(3, 3, 64, 64)),
                lambda: focal_frequency_loss(z(1, 8, 16), z(1, 8, 16)), lambda: focal_frequency_loss(z(1, 16, 1024), z(1, 16, 1024)),
                lambda: focal_frequency_loss(z(1, 48, 16), z(1, 48, 16)), lambda: focal_frequency_loss(z(16, 16), z(16, 16)),
                lambda: focal_frequency_loss(a, b, -1.0), lambda: focal_frequency_loss(a, b, float("nan")),
                lambda: focal_frequency_loss(a, b, True), lambda: focal_frequency_loss(a, b, "1")):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(NotImplementedError):
        focal_frequency_loss(a.cpu(), b.cpu())


def test_a_nan_frame_gets_a_nan_loss_and_leaves_its_neighbours_alone():
    from cdfo_amd.loss import focal_frequency_loss
    sr, hr = cases.case(16, 64, "random-n5")                                    # five frames
    clean = focal_frequency_loss(_dev(sr), _dev(hr))
    bad = np.array(sr)
    bad[3, 7, 11] = float("nan")
    x = _dev(bad).requires_grad_(True)
    loss = focal_frequency_loss(x, _dev(hr))
    loss.sum().backward()
    got, want = loss.detach().cpu().numpy(), clean.cpu().numpy()
    keep = np.arange(5) != 3
    assert np.isnan(got[3]) and np.array_equal(got[keep].view(np.uint32), want[keep].view(np.uint32))
    assert np.isfinite(x.grad.cpu().numpy()[keep]).all()


def test_no_grad_skips_the_inverse_passes(monkeypatch):
    """Asserted by what the wrapper returns: no gradient tensor exists when none is wanted."""
    from cdfo_amd import kernels as K
    from cdfo_amd.loss import focal_frequency_loss
    sr, hr = (_dev(a) for a in cases.case(16, 32, "random-n3"))
    seen, inner = [], K.ffl_loss

    def spy(*a, **kw):
        out = inner(*a, **kw)
        seen.append(out[1])
        return out

    monkeypatch.setattr(K, "ffl_loss", spy)
    plain = focal_frequency_loss(sr, hr)                                    # no input needs a gradient
    with torch.no_grad():
        quiet = focal_frequency_loss(sr.clone().requires_grad_(True), hr)
    only_hr = focal_frequency_loss(sr, hr.clone().requires_grad_(True))
    assert seen == [None, None, None]
    assert not plain.requires_grad and not quiet.requires_grad and not only_hr.requires_grad
    monkeypatch.undo()
    x = sr.clone().requires_grad_(True)
    loud = focal_frequency_loss(x, hr)
    assert loud.requires_grad and torch.equal(loud.detach(), plain) and torch.equal(quiet, plain) and torch.equal(only_hr, plain)


_FITS = {}


def _fit(tag, tmp_path_factory, **kw):
    """(averages, log lines, state dict on the host) of `train.fit` for two epochs of one batch of two 16 x 16 crops (HR 64 x 64) on a
    synthetic set, from the seed 1; run once per tag and shared.  The sizes are those of tests/test_gpu_lpips_loss.py."""
    if tag not in _FITS:
        from arch.SIDECVSR_our import CVSR_V8
        from cdfo_amd.train import fit
        from cdfo_amd.train_data import ClipSet, synthetic_arrays
        clips = ClipSet.from_arrays(*synthetic_arrays(2, 8, 20, 20, seed=1))
        torch.manual_seed(1)
        model, lines = CVSR_V8(SCGs=8).cuda(), []
        averages = fit(model, clips, 2, str(tmp_path_factory.mktemp(tag)), batch_size=2, crop=16, val_itv=10, log=lines.append, **kw)
        _FITS[tag] = averages, lines, {k: v.detach().cpu() for k, v in model.state_dict().items()}
    return _FITS[tag]


def test_fit_with_and_without_the_term(tmp_path_factory):
    a1, l1, s1 = _fit("ffl-a", tmp_path_factory, ffl_weight=2.0, ffl_alpha=1.0)
    a0, l0, s0 = _fit("plain", tmp_path_factory)
    az, lz, sz = _fit("zero", tmp_path_factory, ffl_weight=0.0)
    assert len(a1) == 2 and np.isfinite(a1).all() and len(l1) == 2 and len(l0) == 2
    assert all(bool(torch.isfinite(v).all()) for v in s1.values()) and any(not torch.equal(s1[k], s0[k]) for k in s1)
    for ln, avg in zip(l1, a1):
        m = re.search(r"average epoch loss: ([0-9.]+) \| charbonnier: ([0-9.]+) \| ffl: ([0-9.]+)$", ln)
        assert m and abs(float(m.group(1)) - avg) < 1e-5
        assert float(m.group(3)) > 0 and abs(float(m.group(2)) + 2.0 * float(m.group(3)) - avg) < 1e-3 * avg
    # the plain run: no suffix, and lines and averages are what the keyword's zero gives.  The first epoch's loss is formed before any
    # backward and is equal in every digit; the second follows one step whose flow-warp adjoint adds with fp32 atomics in a plain run
    # (tests/test_gpu_lpips_loss.py), so any two plain runs may differ there in the last digits of an fp32 sum
    assert all(re.search(r"average epoch loss: [0-9.]+$", ln) for ln in l0 + lz)
    strip = lambda lines: [ln.split("] ", 1)[1] for ln in lines]                               # noqa: E731  (the date in front)
    assert strip(l0)[0] == strip(lz)[0] and a0[0] == az[0] and abs(a0[1] - az[1]) <= 1e-5 * a0[1]
    assert strip(l0)[1].split(": ")[:2] == strip(lz)[1].split(": ")[:2]


def test_fit_beside_lpips(tmp_path_factory):
    import lpips_loss_cases
    params = lpips_loss_cases.model(lpips_loss_cases.W1, 21)
    avgs, lines, sd = _fit("ffl-lpips", tmp_path_factory, lpips=params, lpips_weight=0.5, ffl_weight=2.0, ffl_alpha=0.5)
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
    for ln, avg in zip(lines, avgs):
        m = re.search(r"average epoch loss: ([0-9.]+) \| charbonnier: ([0-9.]+) \| lpips: ([0-9.]+) \| ffl: ([0-9.]+)$", ln)
        assert m and abs(float(m.group(1)) - avg) < 1e-5 and float(m.group(3)) > 0 and float(m.group(4)) > 0
        assert abs(float(m.group(2)) + 0.5 * float(m.group(3)) + 2.0 * float(m.group(4)) - avg) < 1e-3 * avg


def test_fit_twice_from_one_seed_gives_equal_weights(tmp_path_factory):
    _, _, s1 = _fit("ffl-a", tmp_path_factory, ffl_weight=2.0, ffl_alpha=1.0)
    _, _, s2 = _fit("ffl-b", tmp_path_factory, ffl_weight=2.0, ffl_alpha=1.0)
    differ = [k for k in s1 if not torch.equal(s1[k], s2[k])]
    print(f"{len(differ)} of {len(s1)} tensors differ between two runs from one seed")
    assert not differ
