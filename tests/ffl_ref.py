"""The focal frequency loss as the project defines it (DESIGN.md "Focal frequency loss"), stated twice.

`statement` is torch: per frame d = sr - hr (ONE fp32 subtraction, part of the definition), F = fft2(d, norm="ortho"), D = Re(F)^2 +
Im(F)^2, M = sqrt(D) ** alpha, w = M / max(M) with NaN -> 0 and a clamp to [0, 1], detached, loss = mean(w D).  It runs in the dtype
it is given: float64 is the reference, float32 (torch.fft in complex64 on the CPU) is the floor the device tests scale their bound by.
`dft_statement` shares no code with it: numpy, the DFT as two matrix products with exp(-2 pi i k n / N) / sqrt(N), no fft call.

Checked in fp64 when tests/test_ffl_cpu.py runs (restated from the issue that asked for the loss; the figures are this file's):
  * the two statements agree to 1.5e-13 of max |F|, 3e-14 of the loss and 1.7e-13 of max |g| over every shape, case and alpha of
    tests/ffl_cases.py, the worst at length 512 (asserted at 1e-11: the DFT product adds n terms per bin where the FFT adds log n);
  * `gradient` -- 2 / (H W) Re(ifft2(w F, norm="ortho")) -- against autograd of `statement`: the difference is 0.0 over all of
    those (asserted at 1e-13 of max |g|: another torch build may order the same operations differently);
  * d = A cos(2 pi (3 y / H + 5 x / W)) gives A^2 / 2; a constant c gives c^2; A (-1)^x gives A^2; alpha = 0 gives mean(d^2) and the
    gradient 2 d / (H W) (Parseval: every bin weighs 1); sr == hr gives exactly 0 and an all-zero gradient, the 0 / 0 weight
    becoming 0 by the NaN rule."""
import numpy as np
import torch


def difference(sr, hr) -> torch.Tensor:
    """fp32 [N,H,W]: the one fp32 subtraction the definition starts from."""
    a, b = (torch.from_numpy(np.array(t)) for t in (sr, hr))
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape == b.shape and a.dim() == 3
    return a - b


def spectrum(d: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    return torch.fft.fft2(d.to(dtype), norm="ortho")


def weights(F: torch.Tensor, alpha: float) -> torch.Tensor:
    D = F.real ** 2 + F.imag ** 2
    M = torch.sqrt(D) ** alpha
    w = M / M.amax(dim=(-2, -1), keepdim=True)
    w = torch.where(torch.isnan(w), torch.zeros_like(w), w)
    return torch.clamp(w, 0.0, 1.0).detach()


def statement(d: torch.Tensor, alpha: float, dtype=torch.float64) -> torch.Tensor:
    """[N] in ``dtype``: the loss of each frame of the fp32 difference ``d`` (differentiable by ``d``)."""
    F = spectrum(d, dtype)
    D = F.real ** 2 + F.imag ** 2
    return (weights(F, alpha) * D).mean(dim=(-2, -1))


def gradient(d: torch.Tensor, alpha: float, dtype=torch.float64) -> torch.Tensor:
    """[N,H,W] in ``dtype``: d loss_n / d sr by the closed form, 2 / (H W) Re(ifft2(w F, norm="ortho"))."""
    F = spectrum(d, dtype)
    return 2.0 / (d.shape[-2] * d.shape[-1]) * torch.fft.ifft2(weights(F, alpha) * F, norm="ortho").real


def autograd_gradient(d: torch.Tensor, alpha: float) -> torch.Tensor:
    x = d.to(torch.float64).requires_grad_(True)
    statement(x, alpha).sum().backward()
    return x.grad


def _dft(n: int) -> np.ndarray:
    k = np.arange(n, dtype=np.float64)
    return np.exp(-2j * np.pi * np.outer(k, k) / n) / np.sqrt(n)


def dft_statement(sr, hr, alpha: float):
    """(F complex128 [N,H,W], loss fp64 [N], g fp64 [N,H,W]) by DFT-matrix products in numpy."""
    a, b = np.asarray(sr), np.asarray(hr)
    assert a.dtype == np.float32 and b.dtype == np.float32
    d = (a - b).astype(np.float64)
    N, H, W = d.shape
    Ah, Aw = _dft(H), _dft(W)
    F = Ah @ d @ Aw.T
    D = F.real ** 2 + F.imag ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        M = np.sqrt(D) ** alpha
        w = M / M.max(axis=(1, 2), keepdims=True)
    w = np.clip(np.where(np.isnan(w), 0.0, w), 0.0, 1.0)
    loss = (w * D).sum(axis=(1, 2)) / (H * W)
    g = 2.0 / (H * W) * (Ah.conj() @ (w * F) @ Aw.conj().T).real
    return F, loss, g
