"""The kernels of the focal frequency loss (csrc/ffl.hip) one entry point at a time through the C ABI, on NaN-prefilled outputs,
against the fp64 statement of tests/ffl_ref.py on the cases of tests/ffl_cases.py; every launch runs twice for equal bits.  The
bound of a shape is 16 x the fp32 floor measured when the test runs (ffl_cases.floors).

Worst measured / bound on the MI355X over the 60 cases (each test prints its own): the spectrum 0.093 (errors 0.8e-7 .. 2.3e-7 of
max |F| against floors of 1.3e-7 .. 2.2e-7), the inverse of the forward 0.128 (1.9e-7 .. 8.0e-7 of max |g| against 2.8e-7 ..
4.4e-7), both at 16x256-patterns: the device is within 2.1 x the fp32 floor everywhere."""
import numpy as np
import pytest
import torch

import ffl_cases as cases

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _lib():
    from cdfo_amd import _lib as L
    return L.lib(), L._vp


def _stream():
    return torch.cuda.current_stream().cuda_stream


_TABLES = {}


def _tw(n):
    from cdfo_amd.kernels import ffl_twiddles
    if n not in _TABLES:
        _TABLES[n] = torch.from_numpy(ffl_twiddles(n)).cuda()
    return _TABLES[n]


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def spectrum(sr, hr):
    """(F fp32 [N,H,W,2], pmax fp64 [N,P]) of cdfo_ffl_spectrum on device tensors, the outputs prefilled with NaN."""
    lib, vp = _lib()
    N, H, W = sr.shape
    P = lib.cdfo_ffl_tiles(H, W)
    F = torch.full((N, H, W, 2), NAN, dtype=torch.float32, device="cuda")
    pmax = torch.full((N, P), NAN, dtype=torch.float64, device="cuda")
    assert lib.cdfo_ffl_spectrum(vp(sr), vp(hr), N, H, W, vp(_tw(H)), vp(_tw(W)), vp(F), vp(pmax), N * P, _stream()) == 0
    return F, pmax


def weight(F, pmax, alpha, apply):
    """(loss fp32 [N]) of cdfo_ffl_weight; F is overwritten when ``apply``."""
    lib, vp = _lib()
    N, H, W, _ = F.shape
    S = lib.cdfo_ffl_strips(H, W)
    partial = torch.full((N, S), NAN, dtype=torch.float64, device="cuda")
    loss = torch.full((N,), NAN, dtype=torch.float32, device="cuda")
    assert lib.cdfo_ffl_weight(vp(F), vp(pmax), pmax.shape[1], N, H, W, alpha, int(apply), vp(partial), N * S, vp(loss), _stream()) == 0
    return loss


def inverse(F):
    """g fp32 [N,H,W] of cdfo_ffl_inverse; F is overwritten."""
    lib, vp = _lib()
    N, H, W, _ = F.shape
    g = torch.full((N, H, W), NAN, dtype=torch.float32, device="cuda")
    assert lib.cdfo_ffl_inverse(vp(F), N, H, W, vp(_tw(H)), vp(_tw(W)), vp(g), _stream()) == 0
    return g


def _complex(F):
    a = F.cpu().numpy()
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


def _bits(t):
    return t.cpu().numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint64)


def _d64(F):
    """re^2 + im^2 of fp32 bins in fp64: both squares are exact, the sum rounds once, as in the kernels."""
    a = F.cpu().numpy().astype(np.float64)
    return a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]


@pytest.mark.parametrize("c", cases.CASES, ids=cases.case_id)
def test_spectrum(c):
    h, w, kind = c
    sr, hr = (_dev(a) for a in cases.case(*c))
    F64, _, _ = cases.reference(h, w, kind, 1.0)
    F, pmax = spectrum(sr, hr)
    F2, pmax2 = spectrum(sr, hr)
    assert np.array_equal(_bits(F), _bits(F2)) and np.array_equal(_bits(pmax), _bits(pmax2))
    err, bound = cases.spectrum_err(_complex(F), F64).max(), cases.MARGIN * cases.floors(h, w)[0]
    print("%s: spectrum %.3g of max |F|, bound %.3g, measured / bound %.3f" % (cases.case_id(c), err, bound, err / bound))
    assert err <= bound
    # the tiles' maxima: every one written, and their maximum is the frame's largest D of the rounded bins, bit for bit
    pm = pmax.cpu().numpy()
    assert np.isfinite(pm).all() and np.array_equal(pm.max(axis=1), _d64(F).max(axis=(1, 2)))


@pytest.mark.parametrize("c", cases.CASES, ids=cases.case_id)
def test_inverse_of_forward_returns_the_difference(c):
    """With every weight 1 (alpha = 0) the inverse of the forward is 2 d / (H W)."""
    h, w, kind = c
    sr, hr = cases.case(*c)
    want = 2.0 * (sr - hr).astype(np.float64) / (h * w)
    F, _ = spectrum(_dev(sr), _dev(hr))
    g, g2 = inverse(F.clone()), inverse(F.clone())
    assert np.array_equal(_bits(g), _bits(g2))
    err, bound = cases.grad_err(g.cpu().numpy(), want).max(), cases.MARGIN * cases.floors(h, w)[2]
    print("%s: inverse of forward %.3g of max |g|, bound %.3g, measured / bound %.3f" % (cases.case_id(c), err, bound, err / bound))
    assert err <= bound


@pytest.mark.parametrize("alpha", cases.ALPHAS)
@pytest.mark.parametrize("c", cases.CASES, ids=cases.case_id)
def test_weight_pass_on_the_statements_spectrum(c, alpha):
    """Fed the fp64 statement's F rounded to fp32 and that F's largest D, the pass is fp64 throughout with one rounding at the end:
    the loss is within 2^-23 of the same sum formed on the host (one fp32 rounding, 2^-24, and the order of fp64 additions), and
    each component of w F within 2^-23 of itself (one rounding, and a last-bit difference of `pow` that may move it) plus 2^-126: a
    product below fp32's normal range -- a noise bin of a pattern's spectrum times its own tiny weight -- has no relative precision."""
    h, w, kind = c
    F64, _, _ = cases.reference(h, w, kind, alpha)
    Fh = np.stack((F64.real, F64.imag), axis=-1).astype(np.float32)
    F = torch.from_numpy(Fh).cuda()
    D = _d64(F)
    pmax = torch.from_numpy(D.max(axis=(1, 2))[:, None].copy()).cuda()
    with np.errstate(invalid="ignore", divide="ignore"):
        M = np.sqrt(D) ** alpha
        wt = M / M.max(axis=(1, 2), keepdims=True)
    wt = np.clip(np.where(np.isnan(wt), 0.0, wt), 0.0, 1.0)
    want = (wt * D).sum(axis=(1, 2)) / (h * w)
    keep = F.clone()
    loss = weight(F, pmax, alpha, False)
    assert np.array_equal(_bits(F), _bits(keep))                             # without `apply` the spectrum is read only
    loss2 = weight(F, pmax, alpha, True)
    assert np.array_equal(_bits(loss), _bits(loss2))
    got = loss.cpu().numpy().astype(np.float64)
    assert (np.abs(got - want) <= 2.0 ** -23 * want).all(), (got, want)
    wF = wt[..., None] * Fh.astype(np.float64)
    assert (np.abs(F.cpu().numpy().astype(np.float64) - wF) <= 2.0 ** -23 * np.abs(wF) + 2.0 ** -126).all()
    F3 = keep.clone()
    weight(F3, pmax, alpha, True)
    assert np.array_equal(_bits(F3), _bits(F))


@pytest.mark.parametrize("shape", [(32, 128), (512, 16), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_a_frame_does_not_reach_its_neighbours(shape):
    """The second and later frames keep their bits in every output when the first frame's contents change, a NaN included."""
    h, w = shape
    rs = np.random.RandomState(5)
    sr, hr = (rs.uniform(0, 1, (3, h, w)).astype(np.float32) for _ in range(2))

    def run(first):
        a = sr.copy()
        a[0] = first
        F, pmax = spectrum(_dev(a), _dev(hr))
        spec = F.clone()
        loss = weight(F, pmax, 1.0, True)
        return spec, pmax, loss, inverse(F)

    base = run(sr[0])
    other = rs.uniform(0, 4, (h, w)).astype(np.float32)
    poisoned = other.copy()
    poisoned[h // 2, w // 3] = NAN
    for first in (other, poisoned):
        for a, b in zip(base, run(first)):
            assert np.array_equal(_bits(a)[1:], _bits(b)[1:]) and not np.array_equal(_bits(a)[0], _bits(b)[0])
    assert np.isnan(run(poisoned)[2].cpu().numpy()[0])
