"""PSNR / SSIM of single-channel frames on the device, with the reference's semantics (metric/psnr_ssim.py:278-317,
320-399, and the per-frame loop of cal_psnr_ssim at :446-484): 0..255 scale, ``crop_border`` pixels dropped, fp64 sums.

The reference saves the network output as an 8-bit PNG, reads it back and compares with the ground-truth PNG; here the
tensors stay in HBM.  ``from_unit_range=True`` multiplies by 255 and clamps (the network emits [0,1] values);
``round8=True`` additionally rounds to the nearest integer.  (The reference's PNG round trip does NOT round: its writer is
``(clamp(out,0,1).numpy() * 255.0).astype(np.uint8)``, test_LD_37.py:179-180, a truncation.  The 8-bit path -- ``kernels.finish_frames``
with ``mode="trunc"``, then ``psnr_u8`` / ``ssim_u8`` below -- has the writer's semantics.)

``psnr_u8`` / ``ssim_u8`` compare two stacks of 8-bit frames over their common size (``cal_psnr_ssim``'s min_height / min_width,
psnr_ssim.py:462-468).  PSNR is formed on the host in fp64 from the exact integer sum of squared differences, which makes it
bit-identical to the fp64 restatement of the reference's calculate_psnr on the same integers.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .kernels import _sample_frames, _stream, _vp, on_device


def _partials(a: torch.Tensor, b: torch.Tensor, crop: int, metric: int, from_unit_range: bool, round8: bool):
    if not (a.is_cuda and b.is_cuda):
        raise NotImplementedError("cdfo_amd.metrics: device tensors only (HIP path, no CPU fallback)")
    if a.shape != b.shape:
        raise ValueError(f"Image shapes are different: {tuple(a.shape)}, {tuple(b.shape)}.")
    H, W = a.shape[-2], a.shape[-1]
    a = a.reshape(-1, H, W).contiguous().float()
    b = b.reshape(-1, H, W).contiguous().float()
    N = a.shape[0]
    part = torch.empty((N, 1024), dtype=torch.float64, device=a.device)
    nb = C.c_int(0)
    with on_device(a):
        _lib.check(_lib.lib().cdfo_metric_partials(_vp(a), _vp(b), N, H, W, crop,
                                                   C.c_float(255.0 if from_unit_range else 1.0), int(from_unit_range),
                                                   int(round8), metric, _vp(part), part.numel(), C.byref(nb), _stream()),
                   "cdfo_metric_partials")
    # the kernel packs its partial sums as [N][nblocks]; fixed-order fp64 sum per frame
    return part.view(-1)[:N * nb.value].view(N, nb.value).sum(dim=1), H - 2 * crop, W - 2 * crop


def calculate_psnr(img1: torch.Tensor, img2: torch.Tensor, crop_border: int = 4, from_unit_range: bool = True,
                   round8: bool = False) -> torch.Tensor:
    """Per-frame PSNR (fp64 tensor [N]); ``inf`` where the frames are identical."""
    s, Hc, Wc = _partials(img1, img2, crop_border, 0, from_unit_range, round8)
    mse = s / float(Hc * Wc)
    return torch.where(mse == 0, torch.full_like(mse, float("inf")), 20.0 * torch.log10(255.0 / torch.sqrt(mse)))


def calculate_ssim(img1: torch.Tensor, img2: torch.Tensor, crop_border: int = 4, from_unit_range: bool = True,
                   round8: bool = False) -> torch.Tensor:
    """Per-frame SSIM (fp64 tensor [N]): mean of the 11x11-Gaussian SSIM map over its valid positions."""
    s, Hc, Wc = _partials(img1, img2, crop_border, 1, from_unit_range, round8)
    return s / float((Hc - 10) * (Wc - 10))


def common_size(h1: int, w1: int, h2: int, w2: int):
    """The size two frames are compared over: psnr_ssim.py:462-468 crops both to (min_height, min_width)."""
    return min(h1, h2), min(w1, w2)


def psnr_from_sse(sse, n: int, peak: int = 255) -> np.ndarray:
    """fp64 [N] PSNR from integer sums of squared differences over n pixels each: calculate_psnr's arithmetic on the host
    (mse = sum / n in fp64; inf where it is 0, else 20 log10(255 / sqrt(mse))).  ``peak``: the samples' largest value, 2**depth - 1,
    in place of 255."""
    mse = np.asarray(sse, dtype=np.int64).astype(np.float64).reshape(-1) / n
    peak = float(peak)
    # frame by frame on numpy scalars: the very expression of calculate_psnr
    return np.array([np.inf if m == 0 else 20.0 * np.log10(peak / np.sqrt(m)) for m in mse], dtype=np.float64)


def _partials_samples(a: torch.Tensor, b: torch.Tensor, crop: int, kind: torch.dtype, which: int):
    """Per-frame sums over the common size of two stacks of ``kind`` samples, and what is left of it inside the border.  uint8:
    cdfo_metric_partials_u8, ``which`` its metric (0: squared differences, 1: the SSIM map); uint16: cdfo_ssim_partials_u16, ``which``
    the peak."""
    a, N, Ha, Wa, pa, sa = _sample_frames(a, "img1", kind)
    b, Nb, Hb, Wb, pb, sb = _sample_frames(b, "img2", kind)
    if N != Nb or a.device != b.device:
        raise ValueError(f"the two stacks must hold the same number of frames on one device, got {N} and {Nb}")
    part = torch.empty((N, 1024), dtype=torch.float64, device=a.device)
    nb = C.c_int(0)
    entry = "cdfo_metric_partials_u8" if kind == torch.uint8 else "cdfo_ssim_partials_u16"
    with on_device(a):
        _lib.check(getattr(_lib.lib(), entry)(_vp(a), pa, C.c_longlong(sa), Ha, Wa, _vp(b), pb, C.c_longlong(sb), Hb, Wb, N, int(crop),
                                              which, _vp(part), part.numel(), C.byref(nb), _stream()), entry)
    Hm, Wm = common_size(Ha, Wa, Hb, Wb)
    return part.view(-1)[:N * nb.value].view(N, nb.value).sum(dim=1), Hm - 2 * crop, Wm - 2 * crop


def sse_u8(img1: torch.Tensor, img2: torch.Tensor, crop_border: int = 4):
    """(int64 device tensor [N] of the sums of squared differences, pixels per frame): the exact numerator of `psnr_u8`."""
    s, Hc, Wc = _partials_samples(img1, img2, crop_border, torch.uint8, 0)
    return s.to(torch.int64), Hc * Wc          # sums of integers below 2^53: the fp64 partials are exact


def psnr_u8(img1: torch.Tensor, img2: torch.Tensor, crop_border: int = 4) -> np.ndarray:
    """Per-frame PSNR of uint8 [N,H,W] device stacks (sizes may differ: compared over the common size), fp64 numpy [N] on the
    host; ``inf`` where the frames are identical."""
    s, n = sse_u8(img1, img2, crop_border)
    return psnr_from_sse(s.cpu().numpy(), n)


def ssim_u8(img1: torch.Tensor, img2: torch.Tensor, crop_border: int = 4) -> torch.Tensor:
    """Per-frame SSIM of uint8 [N,H,W] device stacks over their common size (fp64 device tensor [N])."""
    s, Hc, Wc = _partials_samples(img1, img2, crop_border, torch.uint8, 1)
    return s / float((Hc - 10) * (Wc - 10))


def ssim_u16(img1: torch.Tensor, img2: torch.Tensor, crop_border: int, peak: int) -> torch.Tensor:
    """`ssim_u8` for uint16 [N,H,W] device stacks of samples in 0 .. ``peak`` (2**depth - 1): C1 = (0.01 peak)^2, C2 = (0.03 peak)^2.
    There is no ``sse_u16``: the sums of squares come, as integers, from ``kernels.finish_frames`` and ``kernels.chroma_up4``."""
    if isinstance(peak, bool) or not isinstance(peak, int) or not 1 <= peak <= 65535:
        raise ValueError(f"ssim_u16: peak must be an integer in 1 .. 65535, got {peak!r}")
    s, Hc, Wc = _partials_samples(img1, img2, crop_border, torch.uint16, peak)
    return s / float((Hc - 10) * (Wc - 10))
