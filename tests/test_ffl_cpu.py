"""The focal frequency loss without a GPU: the two statements of tests/ffl_ref.py against each other, the closed forms of the
definition, the gradient's closed form against autograd, the twiddle tables, and the argument checks of the new entry points and of
`train.fit`'s new keywords, none of which may reach the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import ffl_cases as cases
import ffl_ref as ref


@pytest.mark.parametrize("shape", cases.SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_two_statements_agree(shape):
    worst = [0.0, 0.0, 0.0]
    for kind in cases.KINDS:
        sr, hr = cases.case(*shape, kind)
        for alpha in cases.ALPHAS:
            F64, l64, g64 = cases.reference(*shape, kind, alpha)
            F, loss, g = ref.dft_statement(sr, hr, alpha)
            g = g * cases.upstream(len(loss)).astype(np.float64)[:, None, None]
            errs = (cases.spectrum_err(F, F64).max(), cases.loss_err(loss, l64).max(), cases.grad_err(g, g64).max())
            worst = [max(a, float(b)) for a, b in zip(worst, errs)]
    print("%dx%d: fft2 against DFT-matrix statement: spectrum %.2g, loss %.2g, gradient %.2g" % (*shape, *worst))
    assert max(worst) <= 1e-11


@pytest.mark.parametrize("shape", [(16, 16), (16, 512), (512, 16), (32, 128), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_gradient_formula_is_autograd_of_the_statement(shape):
    for kind in cases.KINDS:
        d = ref.difference(*cases.case(*shape, kind))
        for alpha in cases.ALPHAS:
            g, ga = ref.gradient(d, alpha).numpy(), ref.autograd_gradient(d, alpha).numpy()
            assert np.abs(g - ga).max() <= 1e-13 * np.abs(ga).max()


@pytest.mark.parametrize("shape", [(16, 16), (16, 128), (256, 32), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_closed_forms(shape):
    h, w = shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    A, c = 0.3, 0.25
    zero = np.zeros((1, h, w), np.float32)
    f32 = lambda a: np.asarray(a, np.float64)[None].astype(np.float32)                       # noqa: E731
    loss = lambda a, alpha=1.0: float(ref.statement(ref.difference(f32(a), zero), alpha)[0])  # noqa: E731
    assert abs(loss(A * np.cos(2 * np.pi * (3 * y / h + 5 * x / w))) - A * A / 2) <= 1e-6 * A * A
    assert abs(loss(np.full((h, w), c)) - c * c) <= 1e-14                                   # 0.25 is exact in fp32
    assert abs(loss(A * (-1.0) ** x) - A * A) <= 1e-6 * A * A
    assert abs(loss(A * (-1.0) ** y) - A * A) <= 1e-6 * A * A
    imp = np.zeros((h, w))
    imp[h // 3, w // 5] = 0.5
    F = ref.spectrum(torch.from_numpy(f32(imp)))
    assert np.allclose(ref.weights(F, 1.0).numpy(), 1.0, rtol=0, atol=1e-12)                 # |F| is flat: every w = 1
    assert abs(loss(imp) - 0.25 / (h * w)) <= 1e-12
    # alpha = 0: every bin weighs 1 (0 ** 0 = 1 too), so Parseval gives mean(d^2) and the gradient 2 d / (H W)
    sr, hr = cases.case(h, w, "random-n3") if (h, w) in cases.SHAPES else cases.case(64, 64, "random-n3")
    d = ref.difference(sr, hr)
    d64 = d.numpy().astype(np.float64)
    l0, g0 = ref.statement(d, 0.0).numpy(), ref.gradient(d, 0.0).numpy()
    assert np.abs(l0 - (d64 ** 2).mean(axis=(1, 2))).max() <= 1e-14
    assert np.abs(g0 - 2 * d64 / d64[0].size).max() <= 1e-15
    # sr == hr: 0 / 0 weights become 0; the loss is exactly 0 and so is the gradient
    for alpha in (1.0, 0.5):
        same = ref.difference(sr, sr)
        assert not ref.statement(same, alpha).numpy().any() and not ref.gradient(same, alpha).numpy().any()
        assert not ref.autograd_gradient(same, alpha).numpy().any()


def test_floors_are_measured_and_plausible():
    for shape in cases.SHAPES:
        fs, fl, fg = cases.floors(*shape)
        print("%dx%d: fp32 floors: spectrum %.2g, loss %.2g, gradient %.2g" % (*shape, fs, fl, fg))
        assert 1e-8 < fs < 1e-6 and 1e-8 < fl < 1e-6 and 1e-8 < fg < 2e-6


@pytest.mark.parametrize("n", cases.LENGTHS)
def test_twiddle_table(n):
    from cdfo_amd.kernels import ffl_twiddles
    t = ffl_twiddles(n)
    k = np.arange(n // 2, dtype=np.float64)
    want = np.exp(2j * np.pi * k / n)
    assert t.dtype == np.float32 and t.shape == (n // 2, 2) and t.flags.c_contiguous
    assert np.array_equal(t[:, 0], want.real.astype(np.float32)) and np.array_equal(t[:, 1], want.imag.astype(np.float32))
    assert t[0, 0] == 1 and t[0, 1] == 0 and t[n // 4, 1] == 1 and abs(t[n // 4, 0]) < 1e-16
    for bad in (8, 1024, 48, 0, -16, 16.0, None):
        with pytest.raises(ValueError):
            ffl_twiddles(bad)


def test_argument_validation_needs_no_gpu():
    """CDFO_EINVAL (-1) from every new entry point before any HIP call: the pointers below are never dereferenced."""
    from cdfo_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(4096)                                                     # non-null, aligned, never touched
    big = 1 << 30
    assert lib.cdfo_ffl_tiles(16, 16) == 1 and lib.cdfo_ffl_tiles(256, 256) == 16 and lib.cdfo_ffl_tiles(512, 16) == 2
    assert lib.cdfo_ffl_tiles(512, 512) == 64 and lib.cdfo_ffl_strips(16, 16) == 1 and lib.cdfo_ffl_strips(64, 64) == 1
    assert lib.cdfo_ffl_strips(64, 128) == 2 and lib.cdfo_ffl_strips(512, 512) == 64
    sizes = [(8, 16), (16, 8), (1024, 16), (16, 1024), (48, 16), (16, 100), (0, 16), (16, -16)]
    for h, w in sizes:
        assert lib.cdfo_ffl_tiles(h, w) == -1 and lib.cdfo_ffl_strips(h, w) == -1
        assert lib.cdfo_ffl_spectrum(p, p, 1, h, w, p, p, p, p, big, None) == -1
        assert lib.cdfo_ffl_weight(p, p, 1, 1, h, w, 1.0, 1, p, big, p, None) == -1
        assert lib.cdfo_ffl_inverse(p, 1, h, w, p, p, p, None) == -1
    for hole in range(6):                                                    # each pointer null in turn
        a = [p] * 6
        a[hole] = None
        assert lib.cdfo_ffl_spectrum(a[0], a[1], 1, 16, 16, a[2], a[3], a[4], a[5], big, None) == -1
    for hole in range(4):
        a = [p] * 4
        a[hole] = None
        assert lib.cdfo_ffl_weight(a[0], a[1], 1, 1, 16, 16, 1.0, 0, a[2], big, a[3], None) == -1
        assert lib.cdfo_ffl_inverse(a[0], 1, 16, 16, a[1], a[2], a[3], None) == -1
    for n in (0, -1, 65536):
        assert lib.cdfo_ffl_spectrum(p, p, n, 16, 16, p, p, p, p, big, None) == -1
        assert lib.cdfo_ffl_weight(p, p, 1, n, 16, 16, 1.0, 0, p, big, p, None) == -1
        assert lib.cdfo_ffl_inverse(p, n, 16, 16, p, p, p, None) == -1
    assert lib.cdfo_ffl_spectrum(p, p, 3, 16, 64, p, p, p, p, 3 * 4 - 1, None) == -1      # pmax: N P = 12 doubles
    assert lib.cdfo_ffl_spectrum(p, p, 3, 512, 64, p, p, p, p, 3 * 8 - 1, None) == -1     # 8-column tiles at H = 512
    assert lib.cdfo_ffl_weight(p, p, 1, 3, 128, 64, 1.0, 0, p, 3 * 2 - 1, p, None) == -1  # partial: N S = 6 doubles
    assert lib.cdfo_ffl_weight(p, p, 0, 1, 16, 16, 1.0, 0, p, big, p, None) == -1         # no maxima
    for alpha in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert lib.cdfo_ffl_weight(p, p, 1, 1, 16, 16, alpha, 0, p, big, p, None) == -1
    assert lib.cdfo_ffl_spectrum(p, p, 1, 16, 16, p, p, C.c_void_p(4100), p, big, None) == -2   # CDFO_EALIGN: F is read as pairs


def test_python_refuses_before_any_device_work(monkeypatch):
    from cdfo_amd import _lib
    from cdfo_amd import kernels as K
    from cdfo_amd.loss import focal_frequency_loss
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was looked up"))
    a = torch.zeros(2, 1, 16, 32)
    with pytest.raises(NotImplementedError):
        focal_frequency_loss(a, a)
    with pytest.raises(ValueError):
        K.ffl_loss(a, a)                                                     # the wrappers take device tensors only
    for alpha in (-1.0, float("nan"), float("inf"), True, "1", None):
        with pytest.raises(ValueError):
            K.ffl_alpha(alpha, "test")
    assert K.ffl_alpha(0, "test") == 0.0 and K.ffl_alpha(0.5, "test") == 0.5
    assert all(K.ffl_size(n) for n in cases.LENGTHS) and not any(K.ffl_size(n) for n in (8, 24, 1024, 16.0, 0, -32))


def test_fit_refuses_before_any_device_work(tmp_path, monkeypatch):
    from cdfo_amd import _lib
    from cdfo_amd.train import fit
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was looked up"))
    for kw in (dict(ffl_weight=-0.5), dict(ffl_weight=float("inf")), dict(ffl_weight=float("nan")), dict(ffl_weight=True),
               dict(ffl_weight="1"), dict(ffl_alpha=0.5), dict(ffl_alpha=0.0), dict(ffl_weight=0.0, ffl_alpha=2.0),
               dict(ffl_weight=1.0, ffl_alpha=-1.0), dict(ffl_weight=1.0, ffl_alpha=float("nan")), dict(ffl_weight=1.0, ffl_alpha=True),
               dict(ffl_weight=1.0, crop=20), dict(ffl_weight=1.0, crop=2), dict(ffl_weight=1.0, crop=256), dict(ffl_weight=1.0, crop=48)):
        with pytest.raises(ValueError, match="ffl"):
            fit(None, None, 1, str(tmp_path / "never"), **kw)
    assert not (tmp_path / "never").exists()
