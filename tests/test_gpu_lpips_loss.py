"""`cdfo_amd.loss.lpips_loss` on the device: the forward is tied to the metric bit for bit, the gradient is held against the fp64
statement's autograd (tests/lpips_loss_ref.py) on the committed cases of tests/lpips_loss_cases.py, whose frames keep clear of every
ReLU and pool kink (tests/test_lpips_loss_cpu.py asserts that), and `train.fit` runs with the term."""
import re

import numpy as np
import pytest
import torch

import lpips_cases as metric_cases
import lpips_loss_cases as cases
import lpips_loss_ref as ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("normalize", [True, False])
def test_forward_has_the_bits_of_the_metric(normalize):
    """On fp32(k) / 255 the float layers are the uint8 layers of k, and the loss is their total rounded once."""
    from cdfo_amd import metrics as M
    from cdfo_amd.loss import lpips_loss
    params = metric_cases.model(metric_cases.NARROW, 11)
    sr, gt = metric_cases.frames((37, 53), (37, 53), 3, 2)
    ksr, kgt = torch.from_numpy(sr).cuda(), torch.from_numpy(gt).cuda()
    # the division on the host: IEEE, correctly rounded (a device-side `/ 255` of torch may multiply by a reciprocal)
    xsr, xgt = (torch.from_numpy(a.astype(np.float32) / np.float32(255)).cuda() for a in (sr, gt))
    want = M.lpips_layers_u8(ksr, kgt, params, normalize=normalize).cpu().numpy()
    got = M.lpips_layers_f32(xsr, xgt, params, normalize=normalize).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and (want > 0).all()
    four = M.lpips_layers_f32(xsr[:, None], xgt[:, None], params, M.lpips_scratch(3, 37, 53, params, "cuda", pairs=2), normalize).cpu().numpy()
    assert np.array_equal(four.view(np.uint64), want.view(np.uint64))
    loss = lpips_loss(xsr[:, None], xgt[:, None], params, normalize)
    assert loss.dtype == torch.float32 and loss.shape == (3,) and not loss.requires_grad
    assert np.array_equal(loss.cpu().numpy(), M.lpips_from_layers(want).astype(np.float32))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_gradient_matches_the_fp64_statement(name):
    """max |g_dev - g_64| / max |g_64| is at most 16 x the floor measured when the test runs: the fp32-trunk statement's gradient
    against the fp64 one.  Worst ratio of the device's error to that floor seen on the MI355X over the six cases: 0.91
    (w2-24x41-n1; the others 0.50 .. 0.88)."""
    from cdfo_amd.loss import lpips_loss
    params, sr, hr, weights = cases.case(name)
    g64, _, floor = cases.gradients(name)
    x = torch.from_numpy(np.array(sr)).cuda()[:, None].requires_grad_(True)
    y = torch.from_numpy(np.array(hr)).cuda()[:, None].requires_grad_(True)
    loss = lpips_loss(x, y, params)
    want = ref.loss(sr, hr, params).detach().numpy()
    assert np.abs(loss.detach().cpu().numpy() - want).max() <= 1e-4 * want.max()
    loss.backward(gradient=torch.from_numpy(np.array(weights)).cuda())
    assert y.grad is None and x.grad.shape == x.shape and x.grad.dtype == torch.float32
    err = cases.err(x.grad[:, 0].cpu().numpy(), g64)
    print(f"{name}: device {err:.3g} of max |g|, fp32 floor {floor:.3g}, ratio {err / floor:.2f}")
    assert err <= 16 * floor


def test_identities():
    from cdfo_amd.loss import lpips_loss
    params, sr, hr, _ = cases.case("w2-17x19-n3")
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    # sr equal to hr in bits: exactly 0, and a gradient that is all zeros although every norm's derivative is there
    x = dev(hr).requires_grad_(True)
    loss = lpips_loss(x, dev(hr), params)
    loss.sum().backward()
    assert not loss.detach().cpu().numpy().any() and not x.grad.cpu().numpy().any()
    # a frame with upstream gradient 0 gets zeros; two backward passes give equal bits
    grads = []
    for _ in range(2):
        x = dev(sr).requires_grad_(True)
        lpips_loss(x, dev(hr), params).backward(gradient=torch.tensor([1.0, 0.0, 0.5], device="cuda"))
        grads.append(x.grad.cpu().numpy())
    assert np.isfinite(grads[0]).all() and grads[0][0].any() and grads[0][2].any() and not grads[0][1].any()
    assert np.array_equal(grads[0].view(np.uint32), grads[1].view(np.uint32))
    # nothing is cast or made contiguous behind the caller's back
    x = dev(sr)
    wide = torch.zeros((3, 17, 24), device="cuda")
    for bad in (lambda: lpips_loss(x.double(), dev(hr), params), lambda: lpips_loss(x, dev(hr).half(), params),
                lambda: lpips_loss(wide[:, :, :19], dev(hr), params), lambda: lpips_loss(x.transpose(1, 2), dev(hr).transpose(1, 2), params),
                lambda: lpips_loss(x, dev(hr)[:2], params), lambda: lpips_loss(x[:, :15], dev(hr)[:, :15], params),
                lambda: lpips_loss(x[:, None].expand(3, 3, 17, 19), dev(hr)[:, None].expand(3, 3, 17, 19), params),
                lambda: lpips_loss(x, dev(hr), {"w0": np.zeros((16, 3, 3, 3))})):
        with pytest.raises(ValueError):
            bad()


_FITS = {}


def _fit(tag, tmp_path_factory, **kw):
    """(averages, log lines, state dict on the host) of `train.fit` for two epochs of one batch of two 16 x 16 crops (HR 64 x 64) on a
    synthetic set, from the seed 1; run once per tag and shared."""
    if tag not in _FITS:
        from arch.SIDECVSR_our import CVSR_V8
        from cdfo_amd.train import fit
        from cdfo_amd.train_data import ClipSet, synthetic_arrays
        clips = ClipSet.from_arrays(*synthetic_arrays(2, 8, 20, 20, seed=1))               # crop 16 needs an origin to draw: frames above 16
        torch.manual_seed(1)
        model, lines = CVSR_V8(SCGs=8).cuda(), []
        averages = fit(model, clips, 2, str(tmp_path_factory.mktemp(tag)), batch_size=2, crop=16, val_itv=10, log=lines.append, **kw)
        _FITS[tag] = averages, lines, {k: v.detach().cpu() for k, v in model.state_dict().items()}
    return _FITS[tag]


def test_fit_with_and_without_the_term(tmp_path_factory):
    params = cases.model(cases.W1, 21)
    a1, l1, s1 = _fit("lpips-a", tmp_path_factory, lpips=params, lpips_weight=0.5)
    a0, l0, s0 = _fit("plain", tmp_path_factory)
    assert len(a1) == 2 and np.isfinite(a1).all() and len(l1) == 2 and len(l0) == 2
    assert all(bool(torch.isfinite(v).all()) for v in s1.values()) and any(not torch.equal(s1[k], s0[k]) for k in s1)
    for ln, avg in zip(l1, a1):
        m = re.search(r"average epoch loss: ([0-9.]+) \| charbonnier: ([0-9.]+) \| lpips: ([0-9.]+)$", ln)
        assert m and abs(float(m.group(1)) - avg) < 1e-5
        assert float(m.group(3)) > 0 and abs(float(m.group(2)) + 0.5 * float(m.group(3)) - avg) < 1e-3 * avg
    assert all(re.search(r"average epoch loss: [0-9.]+$", ln) for ln in l0)                # without the option: no suffix


def test_fit_twice_from_one_seed_gives_equal_weights(tmp_path_factory):
    """Two `fit` runs with the term from one seed leave equal weights.  The loss is bit-reproducible by construction (`test_identities`);
    the model's own backward was not while `flow_warp`'s adjoint scattered with fp32 atomics (11 to 16 of the 261 tensors then
    differed after two epochs, 244 without the term) and is since that scatter adds fixed-point integers
    (cdfo_flow_warp_bwd_fixed, tests/test_gpu_flow_warp_bwd_fixed.py)."""
    params = cases.model(cases.W1, 21)
    _, _, s1 = _fit("lpips-a", tmp_path_factory, lpips=params, lpips_weight=0.5)
    _, _, s2 = _fit("lpips-b", tmp_path_factory, lpips=params, lpips_weight=0.5)
    differ = [k for k in s1 if not torch.equal(s1[k], s2[k])]
    print(f"{len(differ)} of {len(s1)} tensors differ between two runs from one seed")
    assert not differ


def test_fit_refuses_before_any_launch(tmp_path, monkeypatch):
    from cdfo_amd import _lib
    from cdfo_amd.train import fit
    from cdfo_amd.train_data import ClipSet, synthetic_arrays
    clips = ClipSet.from_arrays(*synthetic_arrays(2, 8, 20, 20, seed=1))
    params = cases.model(cases.W1, 21)
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was looked up"))
    for kw in (dict(lpips=params), dict(lpips=params, lpips_weight=float("inf")), dict(lpips=params, lpips_weight=-0.5),
               dict(lpips_weight=0.5), dict(lpips=params, lpips_weight=0.5, crop=3)):
        with pytest.raises(ValueError, match="lpips|LPIPS"):
            fit(None, clips, 1, str(tmp_path), **kw)
