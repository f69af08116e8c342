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

``msssim_u8`` / ``msssim_u16``: five-scale MS-SSIM of such stacks, the project's own definition (DESIGN.md section 5.000000000;
tests/msssim_ref.py is its numpy statement).  The device leaves ten means per frame, the host combines them in fp64.

``niqe_u8``: the reference's no-reference metric (metric/niqe.py) of 8-bit luma frames, against a pristine model the caller brings
(``niqe_params``).  The device leaves 36 features per 96 x 96 block (``niqe_features_u8``), the host forms the score in fp64
(``niqe_from_features``); DESIGN.md has the definition, tests/niqe_ref.py is its numpy statement.

``brisque_u8``: the reference's other live no-reference metric (metric/brisque.py) of such frames, with a support-vector model the
caller brings (``brisque_params``).  The device leaves 36 features per frame (``brisque_features_u8``), the host forms the score in
fp64 (``brisque_from_features``); DESIGN.md has the definition, tests/brisque_ref.py is its numpy statement.

``tof_u8``: the reference's temporal-consistency figure tOF (metric/psnr_ssim.py: calculate_tOF) of two such stacks, ground truth and
result: the mean endpoint distance between their dense Farneback flows (``farneback_u8``; per chunk ``tof_frames_u8``).  The
definition is the project's own, after the algorithm OpenCV documents, with the reference's arguments; cv2 parity is unpinned.
DESIGN.md has the definition, tests/tof_ref.py is its numpy statement.

``lpips_u8``: LPIPS, the learned perceptual distance of a result to its ground truth, on the luma with a VGG-shaped trunk and a model
the caller brings (``lpips_params``; the project ships none).  The trunk runs in fp32 on the matrix cores (``kernels.conv``), the
distance behind the features in fp64; the device leaves five layer values per frame (``lpips_layers_u8``), the host adds them
(``lpips_from_layers``).  The definition is the project's own; parity with the ``lpips`` package is unpinned.  DESIGN.md has the
definition, tests/lpips_ref.py is its torch statement.  ``lpips_layers_f32`` is the same behind a float stem (a sample is x itself), the
forward of the training loss `cdfo_amd.loss.lpips_loss`, whose backward needs `lpips_stem_adjoint` and the adjoint weights packed here.

``niqe_u16``, ``brisque_u16``, ``tof_u16``, ``lpips_u16`` (and the ``*_features_u16``, ``farneback_u16``, ``tof_frames_u16``,
``lpips_layers_u16`` under them): the four on uint16 frames of samples in 0 .. ``peak`` = 2**depth - 1, the project's own definition
(DESIGN.md): the kernels that read samples form 255 v / peak in fp64 (LPIPS' stem v / peak in fp32), everything behind that is the
8-bit form's, scratch objects, tables and host steps included.  Frames 257 k at the peak 65535 give the bits of the frames k.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from collections.abc import Mapping
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from . import kernels as K
from .kernels import _metric_peak, _sample_frames, _stream, _vp, on_device


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


# ---- MS-SSIM: five scales of the luma (DESIGN.md has the definition; the kernels are in csrc/finish.hip) ----
msssim_min_size = 176                                   # level 4 still holds one 11 x 11 window: 176 >> 4 = 11
MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)     # Wang, Simoncelli, Bovik 2003


def msssim_from_components(c) -> np.ndarray:
    """The combined value from the ten means, on the host in fp64: ``c`` [...,5,2] (numpy or a tensor) holds (M_cs, M_ssim) per
    level; -> [...] prod_{j<4} max(M_cs[j], 0)^w[j] * max(M_ssim[4], 0)^w[4]."""
    c = c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)
    c = c.astype(np.float64)
    if c.shape[-2:] != (5, 2):
        raise ValueError(f"components [...,5,2] expected, got {c.shape}")
    m = np.maximum(np.concatenate([c[..., :4, 0], c[..., 4:, 1]], axis=-1), 0.0)
    return np.prod(m ** np.array(MSSSIM_WEIGHTS, dtype=np.float64), axis=-1)


def msssim_region(h1: int, w1: int, h2: int, w2: int, crop: int):
    """(rows, columns) of level 0: the common size less the border.  ValueError below `msssim_min_size`."""
    Hm, Wm = common_size(h1, w1, h2, w2)
    Hc, Wc = Hm - 2 * crop, Wm - 2 * crop
    if min(Hc, Wc) < msssim_min_size:
        raise ValueError(f"MS-SSIM needs at least {msssim_min_size} x {msssim_min_size} samples inside the border for its five "
                         f"scales, crop_border {crop} leaves {Hc} x {Wc} of the common {Hm} x {Wm}")
    return Hc, Wc


class MsssimScratch:
    """What a call of `msssim_components` needs beside its operands, for up to ``frames`` pairs with a level 0 of ``rows`` x ``cols``
    (`msssim_region`): the pyramid scratch, the buffer of partial sums and the five map sizes as a device tensor.  Calls that share
    one must be ordered, which one stream does."""

    def __init__(self, frames: int, rows: int, cols: int, device):
        frames, rows, cols = int(frames), int(rows), int(cols)
        size = int(_lib.lib().cdfo_msssim_pyramid_bytes(rows, cols, frames))
        if size <= 0:
            raise ValueError(f"no MS-SSIM pyramid for {frames} frames of {rows} x {cols}")
        self.pyramid = torch.empty(size // 4, dtype=torch.float32, device=device)
        self.frames, self.rows, self.cols, self.device = frames, rows, cols, self.pyramid.device
        self.partial = torch.empty(frames * 10240, dtype=torch.float64, device=device)     # the library's "always suffices"
        # the divisors are a device tensor: with a host scalar torch multiplies by the rounded reciprocal, and n ones would not average to 1
        self.sizes = torch.tensor([[((rows >> j) - 10) * ((cols >> j) - 10)] for j in range(5)], dtype=torch.float64, device=device)


def msssim_scratch(n: int, rows: int, cols: int, device) -> MsssimScratch:
    """A `MsssimScratch` for ``n`` frame pairs: what `msssim_components` makes per call unless it is handed one."""
    return MsssimScratch(n, rows, cols, device)


def msssim_components(img1: torch.Tensor, img2: torch.Tensor, crop_border: int, peak: int = None,
                      scratch: MsssimScratch = None) -> torch.Tensor:
    """fp64 device tensor [N,5,2]: per frame and level (M_cs, M_ssim), the means of cs and of l * cs over the level's valid map.
    ``peak`` None: uint8 stacks; else uint16 stacks of that peak.  With a ``scratch`` (`msssim_scratch`, for at least N frames of
    this region on this device) nothing here allocates beyond the result or waits for the device."""
    if peak is not None and (isinstance(peak, bool) or not isinstance(peak, int) or not 1 <= peak <= 65535):
        raise ValueError(f"msssim_u16: peak must be an integer in 1 .. 65535, got {peak!r}")
    kind = torch.uint8 if peak is None else torch.uint16
    a, N, Ha, Wa, pa, sa = _sample_frames(img1, "img1", kind)
    b, Nb, Hb, Wb, pb, sb = _sample_frames(img2, "img2", kind)
    if N != Nb or a.device != b.device:
        raise ValueError(f"the two stacks must hold the same number of frames on one device, got {N} and {Nb}")
    crop = int(crop_border)
    Hm, Wm = common_size(Ha, Wa, Hb, Wb)
    Hc, Wc = Hm - 2 * crop, Wm - 2 * crop
    nb = (C.c_int * 5)()
    with on_device(a):
        if scratch is None and min(Hc, Wc) >= msssim_min_size:
            scratch = MsssimScratch(N, Hc, Wc, a.device)
        if scratch is None:                             # a region below the minimum: the library says so
            tail = (None, C.c_longlong(0), _vp(torch.empty(1, dtype=torch.float64, device=a.device)), 1, nb, _stream())
        elif not isinstance(scratch, MsssimScratch) or scratch.device != a.device or scratch.frames < N or \
                (scratch.rows, scratch.cols) != (Hc, Wc):
            raise ValueError(f"scratch: a msssim_scratch for at least {N} frames of {Hc} x {Wc} on {a.device} expected")
        else:
            tail = (_vp(scratch.pyramid), C.c_longlong(4 * scratch.pyramid.numel()), _vp(scratch.partial), scratch.partial.numel(), nb,
                    _stream())
        entry = "cdfo_msssim_partials_u8" if peak is None else "cdfo_msssim_partials_u16"
        _lib.check(getattr(_lib.lib(), entry)(_vp(a), pa, C.c_longlong(sa), Ha, Wa, _vp(b), pb, C.c_longlong(sb), Hb, Wb, N, crop,
                                              *(() if peak is None else (peak,)), *tail), entry)
    # the kernels pack the rows as [N][row]; frame n's holds level 0's (cs, l cs) pairs, then level 1's, ...: fixed-order fp64 sums
    row = 2 * sum(nb)
    rows, at, sums = scratch.partial[:N * row].view(N, row), 0, []
    for j in range(5):
        sums.append(rows[:, 2 * at:2 * (at + nb[j])].reshape(N, nb[j], 2).sum(dim=1))
        at += nb[j]
    return torch.stack(sums, dim=1) / scratch.sizes


def _msssim(img1, img2, crop_border, peak, components):
    c = msssim_components(img1, img2, crop_border, peak)
    x = torch.from_numpy(np.atleast_1d(msssim_from_components(c))).to(c.device)
    return (x, c) if components else x


def msssim_u8(img1: torch.Tensor, img2: torch.Tensor, crop_border: int = 4, components: bool = False):
    """Per-frame MS-SSIM of uint8 [N,H,W] device stacks over their common size less ``crop_border`` (fp64 device tensor [N]; the
    combine runs on the host).  ``components=True``: (that, the fp64 device tensor [N,5,2] of (M_cs, M_ssim) per level);
    ``[:,0,1]`` is `ssim_u8`'s value.  A region below `msssim_min_size` is an error of the library's (invalid argument)."""
    return _msssim(img1, img2, crop_border, None, components)


def msssim_u16(img1: torch.Tensor, img2: torch.Tensor, crop_border: int, peak: int, components: bool = False):
    """`msssim_u8` for uint16 [N,H,W] device stacks of samples in 0 .. ``peak`` (2**depth - 1)."""
    if peak is None:
        raise ValueError("msssim_u16: uint16 samples need their peak (2**depth - 1)")
    return _msssim(img1, img2, crop_border, peak, components)


# ---- NIQE: the reference's no-reference metric on the 8-bit luma (DESIGN.md has the definition; the kernels are in csrc/niqe.hip) ----
NIQE_BLOCK = 96                                         # scale 1's blocks; scale 2's are 48 x 48 of the half image
NIQE_TABLE = 9801
_niqe_host = {}                                         # "window" and "table": built once per process
_niqe_tables = {}                                       # the table on a device: uploaded once per process and device


class NiqeParams(NamedTuple):
    """The pristine model NIQE scores against: the mean [36] and covariance [36,36] of the features of natural images."""
    mu: np.ndarray
    cov: np.ndarray


def niqe_params(source) -> NiqeParams:
    """The pristine model from ``source``: a path to an ``.npz`` with the keys ``mu_prisparam`` [36] and ``cov_prisparam`` [36,36], or to
    a MATLAB ``.mat`` file with them (the reference's niqe_modelparameters.mat; needs scipy), or a pair of arrays, or a `NiqeParams`.
    The project ships NO model file: the published model is the reference's data, so ``source`` is always the caller's.  fp64; the
    shapes are checked, and that the covariance is finite and symmetric."""
    if isinstance(source, (str, os.PathLike)):
        path = os.fspath(source)
        if path.lower().endswith(".mat"):
            try:
                import scipy.io
            except ImportError as e:
                raise ImportError(f"{path}: reading a .mat model needs scipy; convert it to an .npz with the keys mu_prisparam and "
                                  "cov_prisparam") from e
            held = scipy.io.loadmat(path)
        else:
            with np.load(path) as f:
                held = {k: f[k] for k in f.files}
        missing = [k for k in ("mu_prisparam", "cov_prisparam") if k not in held]
        if missing:
            raise ValueError(f"{path}: no {' / '.join(missing)} in the model file")
        mu, cov = held["mu_prisparam"], held["cov_prisparam"]
    else:
        mu, cov = source
    mu, cov = np.array(mu, dtype=np.float64).reshape(-1), np.array(cov, dtype=np.float64)
    if mu.shape != (36,) or cov.shape != (36, 36):
        raise ValueError(f"NIQE model: a mean of 36 values and a covariance [36,36] expected, got {mu.shape} and {cov.shape}")
    if not (np.isfinite(mu).all() and np.isfinite(cov).all()):
        raise ValueError("NIQE model: the mean and the covariance must be finite")
    if not np.allclose(cov, cov.T, rtol=1e-9, atol=1e-12):
        raise ValueError("NIQE model: the covariance is not symmetric")
    return NiqeParams(mu, cov)


def niqe_window() -> np.ndarray:
    """fp64 [7,7]: MATLAB's fspecial('gaussian', 7, 7/6) as the reference builds it -- exp(-(x^2 + y^2) / (2 sigma^2)), entries below
    eps * max zeroed, normalised, then ROUNDED TO fp32 and widened, so it is no separable product."""
    if "window" not in _niqe_host:
        sigma = 7.0 / 6
        y, x = np.ogrid[-3.0:4.0, -3.0:4.0]
        h = np.exp(-(x * x + y * y) / (2.0 * sigma * sigma))
        h[h < np.finfo(np.float64).eps * h.max()] = 0
        h /= h.sum()
        h = h.astype(np.float32).astype(np.float64)
        h.setflags(write=False)
        _niqe_host["window"] = h
    return _niqe_host["window"]


def niqe_table() -> np.ndarray:
    """fp64 [2,9801]: gam, the float32 ``arange(0.2, 10.001, 0.001)`` widened, and r_gam = exp(2 lgamma(2/gam) - lgamma(1/gam) -
    lgamma(3/gam)).  gam comes from torch's arange on the CPU, as the reference's does: it steps in fp32 inside a vector and a fifth of its
    entries are one fp32 ulp away from float32(0.2 + 0.001 k); the alphas among the features are entries of this table."""
    if "table" not in _niqe_host:
        gam = torch.arange(0.2, 10 + 0.001, 0.001, dtype=torch.float32, device="cpu").numpy().astype(np.float64)
        if gam.shape != (NIQE_TABLE,):
            raise RuntimeError(f"the NIQE table has {gam.shape[0]} entries, {NIQE_TABLE} expected")
        r = np.array([math.exp(2 * math.lgamma(2.0 / g) - (math.lgamma(1.0 / g) + math.lgamma(3.0 / g))) for g in gam])
        t = np.stack([gam, r])
        t.setflags(write=False)
        _niqe_host["table"] = t
    return _niqe_host["table"]


def _niqe_table_on(device) -> torch.Tensor:
    device = torch.device(device)
    if device not in _niqe_tables:
        _niqe_tables[device] = torch.from_numpy(niqe_table().copy()).to(device)
    return _niqe_tables[device]


def niqe_region(h: int, w: int):
    """(rows, columns) NIQE runs over: the top-left whole 96 x 96 blocks of an h x w frame.  ValueError below one block."""
    R, Cc = NIQE_BLOCK * (int(h) // NIQE_BLOCK), NIQE_BLOCK * (int(w) // NIQE_BLOCK)
    if R == 0 or Cc == 0:
        raise ValueError(f"NIQE needs at least one {NIQE_BLOCK} x {NIQE_BLOCK} block, the frames are {h} x {w}")
    return R, Cc


class NiqeScratch:
    """What `niqe_features_u8` needs beside its frames, for up to ``frames`` frames with a region of ``rows`` x ``cols`` (`niqe_region`):
    the MSCN maps of both scales, the half image and the sums.  Calls that share one must be ordered, which one stream does."""

    def __init__(self, frames: int, rows: int, cols: int, device):
        frames, rows, cols = int(frames), int(rows), int(cols)
        if frames <= 0 or rows <= 0 or cols <= 0 or rows % NIQE_BLOCK or cols % NIQE_BLOCK:
            raise ValueError(f"no NIQE region of {rows} x {cols} for {frames} frames: whole {NIQE_BLOCK} x {NIQE_BLOCK} blocks expected")
        f64 = lambda n: torch.empty(n, dtype=torch.float64, device=device)
        self.mscn1, self.half, self.mscn2 = f64(frames * rows * cols), f64(frames * rows * cols // 4), f64(frames * rows * cols // 4)
        self.blocks = (rows // NIQE_BLOCK) * (cols // NIQE_BLOCK)
        self.sums = f64(2 * frames * self.blocks * 30)
        self.frames, self.rows, self.cols, self.device = frames, rows, cols, self.mscn1.device


def niqe_scratch(n: int, rows: int, cols: int, device) -> NiqeScratch:
    """A `NiqeScratch` for ``n`` frames: what `niqe_features_u8` makes per call unless it is handed one."""
    return NiqeScratch(n, rows, cols, device)


def niqe_features_u8(frames: torch.Tensor, scratch: NiqeScratch = None) -> torch.Tensor:
    """fp64 device tensor [K,nb,36]: per frame and 96 x 96 block (block (ih, iw) at row iw * nh + ih, the reference's order) the 18
    features of scale 1 and the 18 of scale 2.  ``frames``: uint8 [K,H,W] (or [H,W]) on the device with contiguous rows, read in place
    over their top-left `niqe_region`.  Seven launches on the current stream; with a ``scratch`` (`niqe_scratch`, for at least K frames
    of this region on this device) nothing here allocates beyond the result, and nothing waits for the device."""
    a, N, H, W, _, _ = _sample_frames(frames, "frames", torch.uint8)
    if N == 0:
        raise ValueError("niqe_features_u8: no frames")
    R, Cc = niqe_region(H, W)
    if scratch is None:
        scratch = NiqeScratch(N, R, Cc, a.device)
    elif not isinstance(scratch, NiqeScratch) or scratch.device != a.device or scratch.frames < N or (scratch.rows, scratch.cols) != (R, Cc):
        raise ValueError(f"scratch: a niqe_scratch for at least {N} frames of {R} x {Cc} on {a.device} expected")
    nb, B = scratch.blocks, NIQE_BLOCK
    with on_device(a):
        table, window = _niqe_table_on(a.device), niqe_window()
        out = torch.empty((N, nb, 36), dtype=torch.float64, device=a.device)
        m1 = K.niqe_mscn(a, R, Cc, window, scratch.mscn1[:N * R * Cc].view(N, R, Cc))
        hf = K.niqe_half(a, R, Cc, scratch.half[:N * R * Cc // 4].view(N, R // 2, Cc // 2))
        m2 = K.niqe_mscn(hf, R // 2, Cc // 2, window, scratch.mscn2[:N * R * Cc // 4].view(N, R // 2, Cc // 2))
        s = scratch.sums[:2 * N * nb * 30].view(2, N, nb, 5, 6)
        K.niqe_features(K.niqe_block_sums(m1, B, s[0]), B * B, table, 0, out)
        K.niqe_features(K.niqe_block_sums(m2, B // 2, s[1]), B * B // 4, table, 1, out)
    return out


def niqe_from_features(F, params) -> np.ndarray:
    """fp64 numpy [K] from features [K,nb,36] (or [nb,36] -> a 0-d array), on the host in fp64: with mu the per-column mean over the
    blocks that ignores NaN entries and cov the sample covariance (divisor n - 1) of the blocks WITHOUT a NaN (one such block: the
    zero matrix), sqrt(d pinv((cov_pris + cov) / 2) d^T), d = mu_pris - mu.  NaN where no block is complete.  ``params``: what
    `niqe_params` takes."""
    params = params if isinstance(params, NiqeParams) else niqe_params(params)
    F = F.detach().cpu().numpy() if isinstance(F, torch.Tensor) else np.asarray(F)
    F = F.astype(np.float64)
    if F.ndim not in (2, 3) or F.shape[-1] != 36 or F.shape[-2] == 0:
        raise ValueError(f"features [K,nb,36] expected, got {F.shape}")
    scores = np.full(F.shape[:-2], np.nan, np.float64)
    for at in np.ndindex(*F.shape[:-2]):
        f = F[at]
        nan = np.isnan(f)
        rows = f[~nan.any(axis=1)]
        if len(rows) == 0:
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            mu = np.where(nan, 0.0, f).sum(axis=0) / (~nan).sum(axis=0)
        cov = np.zeros((36, 36), np.float64)
        if len(rows) > 1:
            c = rows - rows.mean(axis=0)
            cov = c.T @ c / (len(rows) - 1)
        d = params.mu - mu
        with np.errstate(invalid="ignore"):
            scores[at] = np.sqrt(d @ np.linalg.pinv((params.cov + cov) / 2) @ d)
    return scores


def niqe_u8(frames: torch.Tensor, params) -> np.ndarray:
    """Per-frame NIQE (lower is better) of uint8 [K,H,W] device frames, fp64 numpy [K] on the host: `niqe_features_u8` on the device,
    `niqe_from_features` on the host.  ``params``: the caller's pristine model (`niqe_params`); the project ships none."""
    params = params if isinstance(params, NiqeParams) else niqe_params(params)
    return np.atleast_1d(niqe_from_features(niqe_features_u8(frames), params))


def niqe_features_u16(frames: torch.Tensor, peak: int, scratch: NiqeScratch = None) -> torch.Tensor:
    """`niqe_features_u8` for uint16 [K,H,W] device frames of samples in 0 .. ``peak`` (2**depth - 1, an integer in 1 .. 65535): the
    two kernels that read samples form x = 255 v / peak in fp64, an exact product and one correctly rounded division, and every
    statement behind x is the 8-bit one (the project's definition above 8 bits; samples above the peak are not clamped).
    The scratch, the table and the launches are `niqe_features_u8`'s; frames 257 k at the peak 65535 give the bits of the frames k."""
    peak = _metric_peak("niqe_features_u16", peak)
    a, N, H, W, _, _ = _sample_frames(frames, "frames", torch.uint16)
    if N == 0:
        raise ValueError("niqe_features_u16: no frames")
    R, Cc = niqe_region(H, W)
    if scratch is None:
        scratch = NiqeScratch(N, R, Cc, a.device)
    elif not isinstance(scratch, NiqeScratch) or scratch.device != a.device or scratch.frames < N or (scratch.rows, scratch.cols) != (R, Cc):
        raise ValueError(f"scratch: a niqe_scratch for at least {N} frames of {R} x {Cc} on {a.device} expected")
    nb, B = scratch.blocks, NIQE_BLOCK
    with on_device(a):
        table, window = _niqe_table_on(a.device), niqe_window()
        out = torch.empty((N, nb, 36), dtype=torch.float64, device=a.device)
        m1 = K.niqe_mscn(a, R, Cc, window, scratch.mscn1[:N * R * Cc].view(N, R, Cc), peak=peak)
        hf = K.niqe_half(a, R, Cc, scratch.half[:N * R * Cc // 4].view(N, R // 2, Cc // 2), peak=peak)
        m2 = K.niqe_mscn(hf, R // 2, Cc // 2, window, scratch.mscn2[:N * R * Cc // 4].view(N, R // 2, Cc // 2))
        s = scratch.sums[:2 * N * nb * 30].view(2, N, nb, 5, 6)
        K.niqe_features(K.niqe_block_sums(m1, B, s[0]), B * B, table, 0, out)
        K.niqe_features(K.niqe_block_sums(m2, B // 2, s[1]), B * B // 4, table, 1, out)
    return out


def niqe_u16(frames: torch.Tensor, peak: int, params) -> np.ndarray:
    """`niqe_u8` for uint16 [K,H,W] device frames of samples in 0 .. ``peak``: `niqe_features_u16`, then `niqe_from_features`."""
    peak = _metric_peak("niqe_u16", peak)
    params = params if isinstance(params, NiqeParams) else niqe_params(params)
    return np.atleast_1d(niqe_from_features(niqe_features_u16(frames, peak), params))


# ---- BRISQUE: the reference's second no-reference metric on the 8-bit luma (DESIGN.md has the definition; csrc/brisque.hip) ----
BRISQUE_MIN = 16                                        # the smallest frame, each way; scale 2 is then 8 x 8
BRISQUE_TABLE = NIQE_TABLE
_brisque_host = {}                                      # "table": built once per process (the window is NIQE's)
_brisque_tables = {}                                    # the table on a device: uploaded once per process and device


class BrisqueParams(NamedTuple):
    """The model BRISQUE scores with: an RBF support-vector regression on the 36 features scaled to -1 .. 1."""
    sv: np.ndarray                  # fp64 [n,36]
    sv_coef: np.ndarray             # fp64 [n]
    feature_ranges: np.ndarray      # fp64 [36,2]: (lo, hi) per feature
    gamma: float
    rho: float


def brisque_params(source) -> BrisqueParams:
    """The model from ``source``: a path to an ``.npz`` with the keys ``sv`` [n,36], ``sv_coef`` [n], ``feature_ranges`` [36,2],
    ``gamma`` and ``rho``, or those five as a sequence, or a `BrisqueParams`.  The project ships NO model: the published one is the
    reference's data, so ``source`` is always the caller's (tools/gen_brisque_fixture.py --model-out writes such a file from a copy
    of the reference).  fp64; the shapes are checked, n >= 1, every number finite, hi != lo in every range."""
    if isinstance(source, (str, os.PathLike)):
        path = os.fspath(source)
        with np.load(path) as f:
            held = {k: f[k] for k in f.files}
        missing = [k for k in BrisqueParams._fields if k not in held]
        if missing:
            raise ValueError(f"{path}: no {' / '.join(missing)} in the model file")
        source = [held[k] for k in BrisqueParams._fields]
    source = tuple(source)
    if len(source) != 5:
        raise ValueError(f"BRISQUE model: sv, sv_coef, feature_ranges, gamma and rho expected, got {len(source)} items")
    sv, coef, ranges, gamma, rho = (np.array(x, dtype=np.float64) for x in source)
    if coef.ndim == 2 and 1 in coef.shape:
        coef = coef.reshape(-1)
    if sv.ndim != 2 or sv.shape[1] != 36 or sv.shape[0] < 1 or coef.shape != (sv.shape[0],) or ranges.shape != (36, 2):
        raise ValueError(f"BRISQUE model: support vectors [n,36] with n >= 1, n coefficients and ranges [36,2] expected, got {sv.shape}, "
                         f"{coef.shape} and {ranges.shape}")
    if gamma.size != 1 or rho.size != 1:
        raise ValueError(f"BRISQUE model: gamma and rho are scalars, got {gamma.shape} and {rho.shape}")
    if not all(np.isfinite(x).all() for x in (sv, coef, ranges, gamma, rho)):
        raise ValueError("BRISQUE model: every number must be finite")
    if (ranges[:, 0] == ranges[:, 1]).any():
        raise ValueError("BRISQUE model: a feature range with hi == lo")
    return BrisqueParams(sv, coef, ranges, float(gamma.reshape(())), float(rho.reshape(())))


def brisque_window() -> np.ndarray:
    """fp64 [7,7]: the reference's fspecial(7, 7/6) rounded to fp32 and widened -- NIQE's window (`niqe_window`)."""
    return niqe_window()


def brisque_table() -> np.ndarray:
    """fp64 [3,9801]: gam and r_gam of `niqe_table`, and r_ggd = exp(lgamma(1/gam) + lgamma(3/gam) - 2 lgamma(2/gam)), the row the
    symmetric fit of the map itself is searched in (the reference's estimate_ggd_param)."""
    if "table" not in _brisque_host:
        gam, r_gam = niqe_table()
        r_ggd = np.array([math.exp(math.lgamma(1.0 / g) + math.lgamma(3.0 / g) - 2 * math.lgamma(2.0 / g)) for g in gam])
        t = np.stack([gam, r_gam, r_ggd])
        t.setflags(write=False)
        _brisque_host["table"] = t
    return _brisque_host["table"]


def _brisque_table_on(device) -> torch.Tensor:
    device = torch.device(device)
    if device not in _brisque_tables:
        _brisque_tables[device] = torch.from_numpy(brisque_table().copy()).to(device)
    return _brisque_tables[device]


def brisque_size(h: int, w: int):
    """(h, w) as ints; ValueError below 16 x 16 (scale 2's half image must hold the 7 x 7 window and the 8 taps' mirror)."""
    h, w = int(h), int(w)
    if h < BRISQUE_MIN or w < BRISQUE_MIN:
        raise ValueError(f"BRISQUE needs frames of at least {BRISQUE_MIN} x {BRISQUE_MIN}, got {h} x {w}")
    return h, w


class BrisqueScratch:
    """What `brisque_features_u8` needs beside its frames, for up to ``frames`` frames of ``h`` x ``w``: the MSCN maps of both scales,
    the half image and the strips' sums.  Calls that share one must be ordered, which one stream does."""

    def __init__(self, frames: int, h: int, w: int, device):
        frames = int(frames)
        h, w = brisque_size(h, w)
        if frames <= 0:
            raise ValueError(f"no BRISQUE scratch for {frames} frames")
        hh, wh = (h + 1) // 2, (w + 1) // 2
        f64 = lambda n: torch.empty(n, dtype=torch.float64, device=device)
        self.mscn1, self.half, self.mscn2 = f64(frames * h * w), f64(frames * hh * wh), f64(frames * hh * wh)
        self.strips = ((h + K.BRISQUE_STRIP - 1) // K.BRISQUE_STRIP, (hh + K.BRISQUE_STRIP - 1) // K.BRISQUE_STRIP)
        self.sums = f64(frames * sum(self.strips) * 30)
        self.frames, self.h, self.w, self.device = frames, h, w, self.mscn1.device


def brisque_scratch(n: int, h: int, w: int, device) -> BrisqueScratch:
    """A `BrisqueScratch` for ``n`` frames: what `brisque_features_u8` makes per call unless it is handed one."""
    return BrisqueScratch(n, h, w, device)


def brisque_features_u8(frames: torch.Tensor, scratch: BrisqueScratch = None) -> torch.Tensor:
    """fp64 device tensor [K,36]: per frame the 18 features of scale 1 and the 18 of scale 2 (half size).  ``frames``: uint8 [K,H,W]
    (or [H,W]) on the device with contiguous rows, read in place, at least 16 x 16.  Seven launches on the current stream whatever K
    is; with a ``scratch`` (`brisque_scratch`, for at least K frames of this size on this device) nothing here allocates beyond the
    result, and nothing waits for the device.  A frame whose fit is undefined (all samples equal; a product map with no sample of one
    sign) gets NaN among its features, where the reference asserts; the other frames of the call are untouched by it."""
    a, N, H, W, _, _ = _sample_frames(frames, "frames", torch.uint8)
    if N == 0:
        raise ValueError("brisque_features_u8: no frames")
    H, W = brisque_size(H, W)
    if scratch is None:
        scratch = BrisqueScratch(N, H, W, a.device)
    elif not isinstance(scratch, BrisqueScratch) or scratch.device != a.device or scratch.frames < N or (scratch.h, scratch.w) != (H, W):
        raise ValueError(f"scratch: a brisque_scratch for at least {N} frames of {H} x {W} on {a.device} expected")
    Hh, Wh = (H + 1) // 2, (W + 1) // 2
    g1, g2 = scratch.strips
    with on_device(a):
        table, window = _brisque_table_on(a.device), brisque_window()
        out = torch.empty((N, 36), dtype=torch.float64, device=a.device)
        m1 = K.brisque_mscn(a, window, scratch.mscn1[:N * H * W].view(N, H, W))
        hf = K.brisque_half(a, scratch.half[:N * Hh * Wh].view(N, Hh, Wh))
        m2 = K.brisque_mscn(hf, window, scratch.mscn2[:N * Hh * Wh].view(N, Hh, Wh))
        s1 = scratch.sums[:N * g1 * 30].view(N, g1, 5, 6)
        s2 = scratch.sums[N * g1 * 30:N * (g1 + g2) * 30].view(N, g2, 5, 6)
        K.brisque_features(K.brisque_sums(m1, s1), H * W, table, 0, out)
        K.brisque_features(K.brisque_sums(m2, s2), Hh * Wh, table, 1, out)
    return out


def brisque_from_features(F, params) -> np.ndarray:
    """fp64 numpy [K] from features [K,36] (or [36] -> a 0-d array), on the host in fp64: z = -1 + 2 (f - lo) / (hi - lo), then
    sum_i coef_i exp(-gamma |z - sv_i|^2) - rho (lower is better).  NaN where a feature is NaN.  ``params``: what `brisque_params`
    takes."""
    params = params if isinstance(params, BrisqueParams) else brisque_params(params)
    F = F.detach().cpu().numpy() if isinstance(F, torch.Tensor) else np.asarray(F)
    F = F.astype(np.float64)
    if F.ndim not in (1, 2) or F.shape[-1] != 36:
        raise ValueError(f"features [K,36] expected, got {F.shape}")
    lo, hi = params.feature_ranges[:, 0], params.feature_ranges[:, 1]
    scores = np.full(F.shape[:-1], np.nan, np.float64)
    for at in np.ndindex(*F.shape[:-1]):
        z = -1.0 + 2.0 * (F[at] - lo) / (hi - lo)
        d = ((z[None, :] - params.sv) ** 2).sum(axis=1)
        scores[at] = (params.sv_coef * np.exp(-params.gamma * d)).sum() - params.rho
    return scores


def brisque_u8(frames: torch.Tensor, params) -> np.ndarray:
    """Per-frame BRISQUE (lower is better) of uint8 [K,H,W] device frames, fp64 numpy [K] on the host: `brisque_features_u8` on the
    device, `brisque_from_features` on the host.  ``params``: the caller's model (`brisque_params`), checked before any device work;
    the project ships none."""
    params = params if isinstance(params, BrisqueParams) else brisque_params(params)
    return np.atleast_1d(brisque_from_features(brisque_features_u8(frames), params))


def brisque_features_u16(frames: torch.Tensor, peak: int, scratch: BrisqueScratch = None) -> torch.Tensor:
    """`brisque_features_u8` for uint16 [K,H,W] device frames of samples in 0 .. ``peak`` (2**depth - 1, an integer in 1 .. 65535):
    the two kernels that read samples form x = 255 v / peak in fp64 as `niqe_features_u16`'s do, the half image filters x itself, and
    every statement behind x is the 8-bit one.  The scratch, the table and the launches are `brisque_features_u8`'s."""
    peak = _metric_peak("brisque_features_u16", peak)
    a, N, H, W, _, _ = _sample_frames(frames, "frames", torch.uint16)
    if N == 0:
        raise ValueError("brisque_features_u16: no frames")
    H, W = brisque_size(H, W)
    if scratch is None:
        scratch = BrisqueScratch(N, H, W, a.device)
    elif not isinstance(scratch, BrisqueScratch) or scratch.device != a.device or scratch.frames < N or (scratch.h, scratch.w) != (H, W):
        raise ValueError(f"scratch: a brisque_scratch for at least {N} frames of {H} x {W} on {a.device} expected")
    Hh, Wh = (H + 1) // 2, (W + 1) // 2
    g1, g2 = scratch.strips
    with on_device(a):
        table, window = _brisque_table_on(a.device), brisque_window()
        out = torch.empty((N, 36), dtype=torch.float64, device=a.device)
        m1 = K.brisque_mscn(a, window, scratch.mscn1[:N * H * W].view(N, H, W), peak=peak)
        hf = K.brisque_half(a, scratch.half[:N * Hh * Wh].view(N, Hh, Wh), peak=peak)
        m2 = K.brisque_mscn(hf, window, scratch.mscn2[:N * Hh * Wh].view(N, Hh, Wh))
        s1 = scratch.sums[:N * g1 * 30].view(N, g1, 5, 6)
        s2 = scratch.sums[N * g1 * 30:N * (g1 + g2) * 30].view(N, g2, 5, 6)
        K.brisque_features(K.brisque_sums(m1, s1), H * W, table, 0, out)
        K.brisque_features(K.brisque_sums(m2, s2), Hh * Wh, table, 1, out)
    return out


def brisque_u16(frames: torch.Tensor, peak: int, params) -> np.ndarray:
    """`brisque_u8` for uint16 [K,H,W] device frames of samples in 0 .. ``peak``: `brisque_features_u16`, then `brisque_from_features`."""
    peak = _metric_peak("brisque_u16", peak)
    params = params if isinstance(params, BrisqueParams) else brisque_params(params)
    return np.atleast_1d(brisque_from_features(brisque_features_u16(frames, peak), params))


# ---- tOF: the distance between the Farneback flows of ground truth and result (DESIGN.md has the definition; csrc/tof.hip) ----
TOF_MIN = K.TOF_MIN                                     # the smallest region, each way
TOF_LEVELS, TOF_WINSIZE, TOF_ITERATIONS, TOF_POLY_N, TOF_POLY_SIGMA = 3, 15, 3, 5, 1.2      # the reference's arguments
_tof_host = {}                                          # the taps per stage and the expansion's kernels: built once per process


def tof_size(h: int, w: int):
    """[(k, h_k, w_k)] for the stages k = L .. 0 of an h x w region, coarsest first: a stage exists while both sides scaled by
    0.5^k stay at least 32, at most three beyond the full size; sizes round half to even.  ValueError below 32 x 32."""
    h, w = int(h), int(w)
    if h < TOF_MIN or w < TOF_MIN:
        raise ValueError(f"tOF needs a region of at least {TOF_MIN} x {TOF_MIN}, got {h} x {w}")
    L, s = 0, 1.0
    for k in range(TOF_LEVELS):
        s *= 0.5
        if w * s < TOF_MIN or h * s < TOF_MIN:
            break
        L = k + 1
    return [(k, int(np.rint(h * 0.5 ** k)), int(np.rint(w * 0.5 ** k))) for k in range(L, -1, -1)]


def tof_taps(k: int) -> np.ndarray:
    """The smoothing taps of stage k: sigma = (2^k - 1) / 2, max(rint(5 sigma) | 1, 3) taps of a normalised Gaussian; [1/4, 1/2, 1/4]
    at sigma = 0."""
    if ("taps", k) not in _tof_host:
        sigma = (1.0 / 0.5 ** k - 1.0) / 2.0
        n = max(int(np.rint(5.0 * sigma)) | 1, 3)
        if sigma == 0.0:
            t = np.array([0.25, 0.5, 0.25])
        else:
            x = np.arange(n, dtype=np.float64) - (n - 1) // 2
            t = np.exp(-(x * x) / (2.0 * sigma * sigma))
            t = t / t.sum()
        t.setflags(write=False)
        _tof_host["taps", k] = t
    return _tof_host["taps", k]


def tof_poly_kernels() -> np.ndarray:
    """fp64 [37]: the expansion's taps g, x g, x^2 g over x = -5 .. 5 (g the normalised Gaussian of sigma 1.2), then the entries
    [1][1], [0][3], [3][3], [5][5] of the inverse Gram matrix of 1, x, y, x^2, y^2, xy under g (x) g -- the ones symmetry leaves."""
    if "poly" not in _tof_host:
        x = np.arange(-TOF_POLY_N, TOF_POLY_N + 1, dtype=np.float64)
        g = np.exp(-(x * x) / (2.0 * TOF_POLY_SIGMA * TOF_POLY_SIGMA))
        g = g / g.sum()
        X, Y = np.meshgrid(x, x)
        basis = np.stack([np.ones_like(X), X, Y, X * X, Y * Y, X * Y]).reshape(6, -1)
        inv = np.linalg.inv((basis * np.outer(g, g).reshape(-1)) @ basis.T)
        k = np.concatenate([g, x * g, x * x * g, [inv[1, 1], inv[0, 3], inv[3, 3], inv[5, 5]]])
        k.setflags(write=False)
        _tof_host["poly"] = k
    return _tof_host["poly"]


class TofScratch:
    """What the Farneback launches need beside their frames, for groups of up to ``pairs`` frame pairs of an ``h`` x ``w`` region:
    per pair two level images, their ten coefficient planes, five planes of normal equations and two flows, all fp64 (21 values per
    pixel and pair), and the strips' sums.  ``nbytes``: its size.  Calls that share one must be ordered, which one stream does."""

    def __init__(self, pairs: int, h: int, w: int, device):
        pairs = int(pairs)
        self.stages = tof_size(h, w)
        if pairs <= 0:
            raise ValueError(f"no tOF scratch for {pairs} pairs")
        h, w = int(h), int(w)
        f64 = lambda n: torch.empty(n, dtype=torch.float64, device=device)
        px = pairs * h * w
        self.img, self.R, self.M, self.flow, self.up = f64(2 * px), f64(10 * px), f64(5 * px), f64(2 * px), f64(2 * px)
        self.partials = f64(pairs * ((h + K.TOF_STRIP - 1) // K.TOF_STRIP))
        self.pairs, self.h, self.w, self.device = pairs, h, w, self.img.device
        self.nbytes = 8 * sum(t.numel() for t in (self.img, self.R, self.M, self.flow, self.up, self.partials))


def tof_scratch(n: int, h: int, w: int, device) -> TofScratch:
    """A `TofScratch` for groups of ``n`` pairs: what `farneback_u8` and `tof_frames_u8` make per call unless they are handed one."""
    return TofScratch(n, h, w, device)


def _tof_scratch_for(scratch, pairs: int, h: int, w: int, device) -> TofScratch:
    if scratch is None:
        return TofScratch(min(pairs, 8), h, w, device)
    if not isinstance(scratch, TofScratch) or scratch.device != device or (scratch.h, scratch.w) != (h, w):
        raise ValueError(f"scratch: a tof_scratch for a region of {h} x {w} on {device} expected")
    return scratch


def _farneback(s: TofScratch, N: int, level, out: torch.Tensor = None) -> torch.Tensor:
    """The stages of N <= s.pairs pairs.  ``level(k, h, w, taps, img)`` fills the level images [N,2,h,w] of stage k.  -> the flow
    [N,h,w,2], in ``out`` or in the scratch (valid until its next use)."""
    kern, flow = tof_poly_kernels(), None
    for k, h, w in s.stages:
        px = N * h * w
        img = s.img[:2 * px].view(N, 2, h, w)
        level(k, h, w, tof_taps(k), img)
        R = K.tof_polyexp(img, kern, s.R[:10 * px].view(N, 2, 5, h, w))
        if flow is not None:
            flow = K.tof_flow_up(flow, h, w, s.up[:2 * px].view(N, h, w, 2))
        M = s.M[:5 * px].view(N, 5, h, w)
        K.tof_matrices(R, flow, M)
        for i in range(TOF_ITERATIONS):
            last = k == 0 and i + 1 == TOF_ITERATIONS
            flow = K.tof_blur_solve(M, out if last and out is not None else s.flow[:2 * px].view(N, h, w, 2))
            if i + 1 < TOF_ITERATIONS:
                K.tof_matrices(R, flow, M)
    return flow


def farneback_u8(prev: torch.Tensor, cur: torch.Tensor, scratch: TofScratch = None) -> torch.Tensor:
    """fp64 device tensor [N,H,W,2]: the dense flow (dx, dy) from ``prev[j]`` to ``cur[j]``, the project's statement of Farneback's
    algorithm with the reference's arguments (pyr_scale 0.5, levels 3, winsize 15, iterations 3, poly_n 5, poly_sigma 1.2, flags 0;
    cv2 parity unpinned).  ``prev``, ``cur``: uint8 [N,H,W] (or [H,W]) on the device with contiguous rows, read in place, at least
    32 x 32.  The pairs go through the launches together, in groups of the ``scratch``'s size (`tof_scratch`)."""
    c, N, H, W, _, _ = _sample_frames(cur, "cur", torch.uint8)
    p, Np, Hp, Wp, _, _ = _sample_frames(prev, "prev", torch.uint8)
    if N == 0 or (Np, Hp, Wp) != (N, H, W) or p.device != c.device:
        raise ValueError(f"farneback_u8: two stacks of one shape on one device expected, got {tuple(p.shape)} and {tuple(c.shape)}")
    tof_size(H, W)
    with on_device(c):
        s = _tof_scratch_for(scratch, N, H, W, c.device)
        out = torch.empty((N, H, W, 2), dtype=torch.float64, device=c.device)
        for g0 in range(0, N, s.pairs):
            g1 = min(g0 + s.pairs, N)
            _farneback(s, g1 - g0, lambda k, h, w, taps, img: K.tof_level(p[g0:g1], c[g0:g1], h, w, taps, out=img), out[g0:g1])
    return out


def tof_frames_u8(gt: torch.Tensor, sr: torch.Tensor, gt_prev: torch.Tensor = None, sr_prev: torch.Tensor = None,
                  scratch: TofScratch = None) -> torch.Tensor:
    """fp64 device tensor [k]: tOF of the k frames of a chunk, the mean over the common top-left region of the endpoint distance
    between the flow (gt[t-1], gt[t]) and the flow (sr[t-1], sr[t]).  ``gt``, ``sr``: uint8 [k,H,W] on the device with contiguous
    rows, of possibly different sizes, the region at least 32 x 32.  ``gt_prev`` / ``sr_prev``: the frame in front of the chunk
    (uint8 [H,W], the size of its stack), or None at the start of a sequence, where frame 0 is its own previous frame (the
    reference's rule; the flow of that pair is computed, it is not zero).  Ground-truth and result pairs share every launch but the
    level images'; a ``scratch`` for 2 k pairs takes the chunk in one group, a smaller one in several; nothing waits for the device."""
    g, k, Hg, Wg, _, _ = _sample_frames(gt, "gt", torch.uint8)
    r, kr, Hr, Wr, _, _ = _sample_frames(sr, "sr", torch.uint8)
    if k == 0 or kr != k or r.device != g.device:
        raise ValueError(f"tof_frames_u8: two stacks of one length on one device expected, got {tuple(g.shape)} and {tuple(r.shape)}")
    H, W = min(Hg, Hr), min(Wg, Wr)
    tof_size(H, W)
    firsts = []
    for name, stack, first in (("gt_prev", g, gt_prev), ("sr_prev", r, sr_prev)):
        if first is None:
            first = stack[0]
        elif not first.is_cuda or first.dtype != torch.uint8 or tuple(first.shape) != tuple(stack.shape[1:]) or first.device != g.device:
            raise ValueError(f"tof_frames_u8: {name} must be a uint8 frame {tuple(stack.shape[1:])} on the stacks' device")
        firsts.append(first[:H, :W])
    g, r = g[:, :H, :W], r[:, :H, :W]
    with on_device(g):
        s = _tof_scratch_for(scratch, 2 * k, H, W, g.device)
        if s.pairs < 2:
            raise ValueError("tof_frames_u8: the scratch must hold at least two pairs")
        out, m = torch.empty(k, dtype=torch.float64, device=g.device), s.pairs // 2
        for f0 in range(0, k, m):
            f1 = min(f0 + m, k)
            n = f1 - f0

            def level(kk, h, w, taps, img):
                for half, (stack, first) in enumerate(((g, firsts[0]), (r, firsts[1]))):
                    dst = img[half * n:(half + 1) * n]
                    if f0 == 0:
                        K.tof_level(stack[:f1], stack[:f1], h, w, taps, first=first, out=dst)
                    else:
                        K.tof_level(stack[f0 - 1:f1 - 1], stack[f0:f1], h, w, taps, out=dst)

            flow = _farneback(s, 2 * n, level)
            K.tof_epe(flow[:n], flow[n:], s.partials[:n * ((H + K.TOF_STRIP - 1) // K.TOF_STRIP)].view(n, -1), out[f0:f1])
    return out


def tof_u8(gt: torch.Tensor, sr: torch.Tensor) -> np.ndarray:
    """Per-frame tOF (lower is better) of two uint8 [T,H,W] device stacks, ground truth and result, fp64 numpy [T] on the host:
    `tof_frames_u8` on the whole sequence, frame 0 against itself."""
    return tof_frames_u8(gt, sr).cpu().numpy()


def farneback_u16(prev: torch.Tensor, cur: torch.Tensor, peak: int, scratch: TofScratch = None) -> torch.Tensor:
    """`farneback_u8` for uint16 [N,H,W] device stacks of samples in 0 .. ``peak`` (2**depth - 1, an integer in 1 .. 65535): the level
    images are formed from x = 255 v / peak in fp64 (an exact product, one correctly rounded division), so the flow is Farneback's on
    the 0 .. 255 scale whatever the depth; every launch behind the level images is `farneback_u8`'s."""
    peak = _metric_peak("farneback_u16", peak)
    c, N, H, W, _, _ = _sample_frames(cur, "cur", torch.uint16)
    p, Np, Hp, Wp, _, _ = _sample_frames(prev, "prev", torch.uint16)
    if N == 0 or (Np, Hp, Wp) != (N, H, W) or p.device != c.device:
        raise ValueError(f"farneback_u16: two stacks of one shape on one device expected, got {tuple(p.shape)} and {tuple(c.shape)}")
    tof_size(H, W)
    with on_device(c):
        s = _tof_scratch_for(scratch, N, H, W, c.device)
        out = torch.empty((N, H, W, 2), dtype=torch.float64, device=c.device)
        for g0 in range(0, N, s.pairs):
            g1 = min(g0 + s.pairs, N)
            _farneback(s, g1 - g0, lambda k, h, w, taps, img: K.tof_level(p[g0:g1], c[g0:g1], h, w, taps, out=img, peak=peak), out[g0:g1])
    return out


def tof_frames_u16(gt: torch.Tensor, sr: torch.Tensor, peak: int, gt_prev: torch.Tensor = None, sr_prev: torch.Tensor = None,
                   scratch: TofScratch = None) -> torch.Tensor:
    """`tof_frames_u8` for uint16 stacks (and carried frames) of samples in 0 .. ``peak``, read as `farneback_u16` reads them; the
    grouping, the scratch and every launch behind the level images are `tof_frames_u8`'s."""
    peak = _metric_peak("tof_frames_u16", peak)
    g, k, Hg, Wg, _, _ = _sample_frames(gt, "gt", torch.uint16)
    r, kr, Hr, Wr, _, _ = _sample_frames(sr, "sr", torch.uint16)
    if k == 0 or kr != k or r.device != g.device:
        raise ValueError(f"tof_frames_u16: two stacks of one length on one device expected, got {tuple(g.shape)} and {tuple(r.shape)}")
    H, W = min(Hg, Hr), min(Wg, Wr)
    tof_size(H, W)
    firsts = []
    for name, stack, first in (("gt_prev", g, gt_prev), ("sr_prev", r, sr_prev)):
        if first is None:
            first = stack[0]
        elif not first.is_cuda or first.dtype != torch.uint16 or tuple(first.shape) != tuple(stack.shape[1:]) or first.device != g.device:
            raise ValueError(f"tof_frames_u16: {name} must be a uint16 frame {tuple(stack.shape[1:])} on the stacks' device")
        firsts.append(first[:H, :W])
    g, r = g[:, :H, :W], r[:, :H, :W]
    with on_device(g):
        s = _tof_scratch_for(scratch, 2 * k, H, W, g.device)
        if s.pairs < 2:
            raise ValueError("tof_frames_u16: the scratch must hold at least two pairs")
        out, m = torch.empty(k, dtype=torch.float64, device=g.device), s.pairs // 2
        for f0 in range(0, k, m):
            f1 = min(f0 + m, k)
            n = f1 - f0

            def level(kk, h, w, taps, img):
                for half, (stack, first) in enumerate(((g, firsts[0]), (r, firsts[1]))):
                    dst = img[half * n:(half + 1) * n]
                    if f0 == 0:
                        K.tof_level(stack[:f1], stack[:f1], h, w, taps, first=first, out=dst, peak=peak)
                    else:
                        K.tof_level(stack[f0 - 1:f1 - 1], stack[f0:f1], h, w, taps, out=dst, peak=peak)

            flow = _farneback(s, 2 * n, level)
            K.tof_epe(flow[:n], flow[n:], s.partials[:n * ((H + K.TOF_STRIP - 1) // K.TOF_STRIP)].view(n, -1), out[f0:f1])
    return out


def tof_u16(gt: torch.Tensor, sr: torch.Tensor, peak: int) -> np.ndarray:
    """`tof_u8` for two uint16 [T,H,W] device stacks of samples in 0 .. ``peak``: `tof_frames_u16` on the whole sequence."""
    return tof_frames_u16(gt, sr, peak).cpu().numpy()


# ---- LPIPS: the learned perceptual distance of result and ground truth, VGG-shaped trunk (DESIGN.md has the definition; csrc/lpips.hip) ----
LPIPS_MIN = K.LPIPS_MIN                                 # the smallest region, each way: stage 5 is then 1 x 1
LPIPS_STAGES = (2, 2, 3, 3, 3)                          # convolutions per stage; a 2 x 2 / 2 max-pool opens stages 2 .. 5
LPIPS_WIDTHS = (64, 128, 256, 512, 512)                 # the published net's stage widths; a model's own are data
LPIPS_TRUNK_KEYS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)     # features.<i> of a VGG16 state dict, in order
LPIPS_CONVS = sum(LPIPS_STAGES)


class LpipsParams:
    """The model LPIPS scores with: the trunk's 13 convolutions and the five per-channel weights of the distance."""

    def __init__(self, weights, biases, lins):
        self.weights = tuple(weights)                   # 13 x fp32 [Cout,Cin,3,3]
        self.biases = tuple(biases)                     # 13 x fp32 [Cout]
        self.lins = tuple(lins)                         # 5 x fp64 [C_k]
        self.widths = tuple(int(l.shape[0]) for l in self.lins)
        self._device = {}                               # the packed model per device: uploaded and packed once

    def arrays(self) -> dict:
        """The model as the mapping `lpips_params` reads: w0 .. w12, b0 .. b12, lin0 .. lin4."""
        d = {f"w{i}": w for i, w in enumerate(self.weights)}
        d.update({f"b{i}": b for i, b in enumerate(self.biases)})
        d.update({f"lin{k}": l for k, l in enumerate(self.lins)})
        return d


def _lpips_state_dict(x, what: str) -> dict:
    """A torch checkpoint (a path, read with torch.load alone, or the state dict itself) as {name: numpy array}."""
    if isinstance(x, (str, os.PathLike)):
        x = torch.load(os.fspath(x), map_location="cpu", weights_only=True)
    if not isinstance(x, Mapping):
        raise ValueError(f"LPIPS model: the {what} must be a state dict or a path to one, got {type(x).__name__}")
    return {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in x.items()}


def lpips_params(source) -> LpipsParams:
    """The model from ``source``: a path to an ``.npz`` with ``w0`` .. ``w12`` ([Cout,Cin,3,3]), ``b0`` .. ``b12`` and ``lin0`` .. ``lin4``
    ([C_k]); a mapping of those arrays; a pair (trunk, head) of torch checkpoints -- paths or state dicts, the trunk with VGG16's
    ``features.{0,2,5,7,10,12,14,17,19,21,24,26,28}.weight`` / ``.bias`` names, the head with ``lin{k}.model.1.weight`` -- or an
    `LpipsParams`.  The project ships NO model (tools/make_lpips_model.py writes the ``.npz`` from a user's checkpoints).  Checked:
    the topology (3 input channels, stages of 2, 2, 3, 3, 3 convolutions of one width each, every input width the width before),
    widths that are multiples of 16 (the first at most 256), one weight per channel in every lin, every number finite."""
    if isinstance(source, LpipsParams):
        return source
    if isinstance(source, (str, os.PathLike)):
        path = os.fspath(source)
        with np.load(path) as f:
            source = {k: f[k] for k in f.files}
    if not isinstance(source, Mapping):
        pair = tuple(source)
        if len(pair) != 2:
            raise ValueError(f"LPIPS model: an .npz, a mapping of its arrays or a (trunk, head) pair of checkpoints expected, got {len(pair)} items")
        trunk, head = _lpips_state_dict(pair[0], "trunk"), _lpips_state_dict(pair[1], "head")
        source = {}
        for i, key in enumerate(LPIPS_TRUNK_KEYS):
            for short, kind in (("w", "weight"), ("b", "bias")):
                if f"features.{key}.{kind}" not in trunk:
                    raise ValueError(f"LPIPS model: no features.{key}.{kind} in the trunk's state dict")
                source[f"{short}{i}"] = trunk[f"features.{key}.{kind}"]
        for k in range(5):
            if f"lin{k}.model.1.weight" not in head:
                raise ValueError(f"LPIPS model: no lin{k}.model.1.weight in the head's state dict")
            source[f"lin{k}"] = head[f"lin{k}.model.1.weight"]
    names = [f"w{i}" for i in range(LPIPS_CONVS)] + [f"b{i}" for i in range(LPIPS_CONVS)] + [f"lin{k}" for k in range(5)]
    missing = [n for n in names if n not in source]
    if missing:
        raise ValueError(f"LPIPS model: no {' / '.join(missing)} in the model")
    ws = [np.ascontiguousarray(source[f"w{i}"], dtype=np.float32) for i in range(LPIPS_CONVS)]
    bs = [np.ascontiguousarray(source[f"b{i}"], dtype=np.float32) for i in range(LPIPS_CONVS)]
    lins = [np.array(source[f"lin{k}"], dtype=np.float64) for k in range(5)]
    cin, i = 3, 0
    for k, convs in enumerate(LPIPS_STAGES):
        width = int(ws[i].shape[0]) if ws[i].ndim == 4 else 0
        if width <= 0 or width % 16 or (k == 0 and width > K.LPIPS_STEM_MAXC):
            raise ValueError(f"LPIPS model: stage {k + 1} has width {width}; widths are multiples of 16 (the first at most "
                             f"{K.LPIPS_STEM_MAXC})")
        for _ in range(convs):
            if ws[i].shape != (width, cin, 3, 3) or bs[i].shape != (width,):
                raise ValueError(f"LPIPS model: convolution {i} of stage {k + 1} must be [{width},{cin},3,3] with {width} biases, got "
                                 f"{ws[i].shape} and {bs[i].shape}")
            cin, i = width, i + 1
        if lins[k].size != width or lins[k].ndim < 1 or max(lins[k].shape) != width:
            raise ValueError(f"LPIPS model: lin{k} must hold {width} weights, got {lins[k].shape}")
        lins[k] = np.ascontiguousarray(lins[k].reshape(-1))
    if not all(np.isfinite(x).all() for x in ws + bs + lins):
        raise ValueError("LPIPS model: every number must be finite")
    for x in ws + bs + lins:
        x.setflags(write=False)
    return LpipsParams(ws, bs, lins)


def lpips_random_params(widths=LPIPS_WIDTHS, seed: int = 0) -> LpipsParams:
    """A He-initialised model of the given stage widths for tests and benchmarks: weights N(0, 2 / (9 Cin)), biases N(0, 0.05^2),
    lin weights uniform in 0 .. 1 / C_k (the published ones are non-negative too).  It measures nothing perceptual."""
    widths = tuple(int(v) for v in widths)
    if len(widths) != 5:
        raise ValueError(f"five stage widths expected, got {widths}")
    rs = np.random.RandomState(seed)
    arrays, cin, i = {}, 3, 0
    for k, convs in enumerate(LPIPS_STAGES):
        for _ in range(convs):
            arrays[f"w{i}"] = (rs.standard_normal((widths[k], cin, 3, 3)) * math.sqrt(2.0 / (9 * cin))).astype(np.float32)
            arrays[f"b{i}"] = (rs.standard_normal(widths[k]) * 0.05).astype(np.float32)
            cin, i = widths[k], i + 1
        arrays[f"lin{k}"] = (rs.uniform(0.0, 1.0, widths[k]) / widths[k]).astype(np.float32)
    return lpips_params(arrays)


def lpips_size(h: int, w: int):
    """[(h_k, w_k)] of the five taps of an h x w region: each stage halves the one before, odd sizes floored.  ValueError below
    16 x 16, where stage 5 would be empty."""
    h, w = int(h), int(w)
    if h < LPIPS_MIN or w < LPIPS_MIN:
        raise ValueError(f"LPIPS needs a region of at least {LPIPS_MIN} x {LPIPS_MIN}, got {h} x {w}")
    return [(h >> k, w >> k) for k in range(5)]


def _lpips_widths(model) -> tuple:
    widths = model.widths if isinstance(model, LpipsParams) else tuple(int(v) for v in model)
    if len(widths) != 5 or min(widths) <= 0 or any(v % 16 for v in widths):
        raise ValueError(f"five stage widths, multiples of 16, expected, got {widths}")
    return widths


class LpipsScratch:
    """What `lpips_layers_u8` needs beside its frames for an ``h`` x ``w`` region and a trunk of the given stage widths: two ping-pong
    fp32 feature buffers, each the largest activation of ``pairs`` (result, ground truth) pairs -- the trunk takes that many pairs per
    pass whatever the chunk's size is -- and the distance's strip sums for up to ``frames`` frames per call.  ``nbytes``: its size
    (`LpipsScratch.bytes_for` gives it without allocating).  Calls that share one must be ordered, which one stream does."""

    @staticmethod
    def _plan(pairs: int, h: int, w: int, widths, frames: int):
        sizes = lpips_size(h, w)
        widths = _lpips_widths(widths)
        pairs, frames = int(pairs), int(frames)
        if pairs <= 0 or frames <= 0:
            raise ValueError(f"no LPIPS scratch for {pairs} pairs per pass and {frames} frames")
        act = 2 * pairs * max(hk * wk * c for (hk, wk), c in zip(sizes, widths))
        strips = tuple((hk + K.LPIPS_STRIP - 1) // K.LPIPS_STRIP for hk, _ in sizes)
        return sizes, widths, pairs, frames, act, strips

    @staticmethod
    def bytes_for(pairs: int, h: int, w: int, widths=LPIPS_WIDTHS, frames: int = 8) -> int:
        _, _, _, frames, act, strips = LpipsScratch._plan(pairs, h, w, widths, frames)
        return 2 * 4 * act + 8 * frames * sum(strips)

    def __init__(self, pairs: int, h: int, w: int, widths, frames: int, device):
        self.sizes, self.widths, self.pairs, self.frames, act, self.strips = self._plan(pairs, h, w, widths, frames)
        self.a = torch.empty(act, dtype=torch.float32, device=device)
        self.b = torch.empty(act, dtype=torch.float32, device=device)
        self.partials = torch.empty(self.frames * sum(self.strips), dtype=torch.float64, device=device)
        self.h, self.w, self.device = int(h), int(w), self.a.device
        self.nbytes = 4 * (self.a.numel() + self.b.numel()) + 8 * self.partials.numel()


def lpips_scratch(n: int, h: int, w: int, model, device, pairs: int = 1) -> LpipsScratch:
    """An `LpipsScratch` for calls of up to ``n`` frames of an ``h`` x ``w`` region: what `lpips_layers_u8` makes per call unless it
    is handed one.  ``model``: an `LpipsParams` or the five stage widths.  ``pairs``: the pairs per pass of the trunk."""
    return LpipsScratch(pairs, h, w, model, n, device)


def _lpips_on(params: LpipsParams, device):
    """The model on a device: the stem's weights as they are, the other twelve convolutions packed by `kernels.pack_conv`, the lin
    weights in fp64.  Built once per model and device."""
    device = torch.device(device)
    if device not in params._device:
        t = lambda a, dt: torch.from_numpy(np.array(a)).to(device=device, dtype=dt).contiguous()
        with torch.cuda.device(device):
            convs = [K.pack_conv(t(w, torch.float32), t(b, torch.float32)) for w, b in zip(params.weights[1:], params.biases[1:])]
        params._device[device] = SimpleNamespace(w0=t(params.weights[0], torch.float32), b0=t(params.biases[0], torch.float32),
                                                 convs=convs, lins=[t(l, torch.float64) for l in params.lins])
    return params._device[device]


def lpips_stem_adjoint(weight0, normalize: bool = True) -> np.ndarray:
    """fp32 [C0,3,3]: the stem's weights [C0,3,3,3] folded over the three scaled channels, ``k sum_c w[o][c][ky][kx] / scale_c`` with
    k = 2 with ``normalize``, else 1, formed in fp64 and rounded once.  The padding of the scaled tensor is constant, so this is all
    the adjoint of the scaling and conv1_1 needs (`kernels.lpips_stem_bwd`)."""
    w = np.asarray(weight0, dtype=np.float64)
    scale = np.array((.458, .448, .450), dtype=np.float64)
    return ((2.0 if normalize else 1.0) * (w / scale[None, :, None, None]).sum(axis=1)).astype(np.float32)


def _lpips_adjoint_on(params: LpipsParams, device):
    """`_lpips_on` with what the backward of `cdfo_amd.loss.lpips_loss` needs beside it, built once per model and device on first use:
    ``adj``, the other twelve convolutions' adjoint weights (flipped and transposed, no bias) packed by `kernels.pack_conv`, and
    ``wf``, the stem's folded weights for both values of ``normalize``."""
    m = _lpips_on(params, device)
    if not hasattr(m, "adj"):
        t = lambda a: torch.from_numpy(np.array(a)).to(device=m.w0.device, dtype=torch.float32)
        with torch.cuda.device(m.w0.device):
            m.wf = {flag: t(lpips_stem_adjoint(params.weights[0], flag)).contiguous() for flag in (False, True)}
            m.adj = [K.pack_conv(t(w).flip(2, 3).transpose(0, 1).contiguous(), None) for w in params.weights[1:]]
    return m


def _lpips_f32_frames(t: torch.Tensor, name: str) -> torch.Tensor:
    """A dense fp32 device tensor [N,1,H,W] or [N,H,W] as [N,H,W]; anything else is a ValueError (nothing is cast or copied)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() \
            or not (t.dim() == 3 or (t.dim() == 4 and t.shape[1] == 1)) or t.shape[0] == 0:
        raise ValueError(f"{name}: a dense fp32 device tensor [N,1,H,W] or [N,H,W] expected, got {getattr(t, 'dtype', type(t))} "
                         f"{tuple(getattr(t, 'shape', ()))}" + (f" strides {t.stride()}" if isinstance(t, torch.Tensor) else ""))
    return t.view(t.shape[0], t.shape[-2], t.shape[-1])


def _lpips_layers_f32(a: torch.Tensor, b: torch.Tensor, params: LpipsParams, scratch: LpipsScratch, normalize: bool, keep=None):
    """`lpips_layers_u8`'s launches behind the float stem on fp32 [N,h,w] stacks of one shape.  ``keep(i, x, n)``: called behind
    convolution ``i`` (0 .. 12) with its output ``x`` [2 n,...], the result's frames first; the buffer is reused two launches on."""
    N, h, w = a.shape
    sizes, widths, strips = scratch.sizes, scratch.widths, scratch.strips
    with on_device(a):
        m = _lpips_on(params, a.device)
        partials = scratch.partials[:N * sum(strips)]
        first = [N * sum(strips[:k]) for k in range(5)]
        for g0 in range(0, N, scratch.pairs):
            g1 = min(g0 + scratch.pairs, N)
            n = g1 - g0
            act = lambda buf, k, c: buf[:2 * n * sizes[k][0] * sizes[k][1] * c].view(2 * n, sizes[k][0], sizes[k][1], c)
            cur, other = scratch.a, scratch.b
            x = act(cur, 0, widths[0])
            K.lpips_stem_f32(a[g0:g1], m.w0, m.b0, normalize, out=x[:n])
            K.lpips_stem_f32(b[g0:g1], m.w0, m.b0, normalize, out=x[n:])
            if keep is not None:
                keep(0, x, n)
            i = 0
            for k, convs in enumerate(LPIPS_STAGES):
                if k:
                    x = K.lpips_pool2(x, act(other, k, widths[k - 1]))
                    cur, other = other, cur
                for _ in range(convs - (k == 0)):
                    x = K.conv(x, m.convs[i], pad=1, act=K.ACT_RELU, prec=K.PREC_F32, out=act(other, k, widths[k]))
                    cur, other = other, cur
                    i += 1
                    if keep is not None:
                        keep(i, x, n)
                K.lpips_dist(x[:n], x[n:], m.lins[k], partials[first[k]:first[k] + N * strips[k]].view(N, strips[k])[g0:g1])
        return K.lpips_fold(partials, N, strips, [hk * wk for hk, wk in sizes])


def lpips_layers_f32(sr: torch.Tensor, hr: torch.Tensor, params, scratch: LpipsScratch = None, normalize: bool = True) -> torch.Tensor:
    """`lpips_layers_u8` for float frames, the forward of the training loss (`cdfo_amd.loss.lpips_loss`): fp64 device tensor [N,5].
    ``sr``, ``hr``: dense fp32 device tensors [N,1,H,W] or [N,H,W] of ONE shape, H, W >= 16; a sample is used as x itself, nominally
    in 0 .. 1: no / 255, no clamp, no quantisation.  Behind that load every launch is `lpips_layers_u8`'s, so frames fp32(k) / 255
    give the bits of the uint8 frames k."""
    a, b = _lpips_f32_frames(sr, "lpips_layers_f32: sr"), _lpips_f32_frames(hr, "lpips_layers_f32: hr")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"lpips_layers_f32: two stacks of one shape on one device expected, got {tuple(sr.shape)} and {tuple(hr.shape)}")
    N, h, w = (int(v) for v in a.shape)
    lpips_size(h, w)
    params = lpips_params(params)
    widths = params.widths
    if scratch is None:
        scratch = LpipsScratch(1, h, w, widths, N, a.device)
    elif not isinstance(scratch, LpipsScratch) or scratch.device != a.device or (scratch.h, scratch.w) != (h, w) \
            or scratch.widths != widths or scratch.frames < N:
        raise ValueError(f"scratch: an lpips_scratch for at least {N} frames of a {h} x {w} region and widths {widths} on {a.device} expected")
    return _lpips_layers_f32(a, b, params, scratch, bool(normalize))


def lpips_layers_u8(sr: torch.Tensor, gt: torch.Tensor, params, scratch: LpipsScratch = None, normalize: bool = True) -> torch.Tensor:
    """fp64 device tensor [N,5]: per frame the five layer distances d_k of ``sr[j]`` to ``gt[j]`` over their common top-left region
    (no border dropped), whose sum is LPIPS.  ``sr``, ``gt``: uint8 [N,H,W] (or [H,W]) on the device with contiguous rows, of possibly
    different sizes, read in place; the region at least 16 x 16.  ``params``: what `lpips_params` takes.  ``normalize``: samples to
    -1 .. 1 before the trunk's scaling (the default, and what the evaluators use); False feeds v / 255.  Result and ground truth of
    ``scratch.pairs`` frames go through the trunk as ONE batch, so equal frames see equal arithmetic and score exactly 0; every
    convolution writes into the scratch, and with a ``scratch`` (`lpips_scratch`) nothing here allocates beyond the result and
    nothing waits for the device.  A pass is 2 + 12 + 4 + 5 launches, the call one more."""
    a, N, Ha, Wa, _, _ = _sample_frames(sr, "sr", torch.uint8)
    b, Nb, Hb, Wb, _, _ = _sample_frames(gt, "gt", torch.uint8)
    if N == 0 or Nb != N or a.device != b.device:
        raise ValueError(f"lpips_layers_u8: two stacks of one length on one device expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    h, w = min(Ha, Hb), min(Wa, Wb)
    sizes = lpips_size(h, w)
    params = lpips_params(params)
    widths = params.widths
    if scratch is None:
        scratch = LpipsScratch(1, h, w, widths, N, a.device)
    elif not isinstance(scratch, LpipsScratch) or scratch.device != a.device or (scratch.h, scratch.w) != (h, w) \
            or scratch.widths != widths or scratch.frames < N:
        raise ValueError(f"scratch: an lpips_scratch for at least {N} frames of a {h} x {w} region and widths {widths} on {a.device} expected")
    a, b = a[:, :h, :w], b[:, :h, :w]
    strips = scratch.strips
    with on_device(a):
        m = _lpips_on(params, a.device)
        partials = scratch.partials[:N * sum(strips)]
        first = [N * sum(strips[:k]) for k in range(5)]
        for g0 in range(0, N, scratch.pairs):
            g1 = min(g0 + scratch.pairs, N)
            n = g1 - g0
            act = lambda buf, k, c: buf[:2 * n * sizes[k][0] * sizes[k][1] * c].view(2 * n, sizes[k][0], sizes[k][1], c)
            cur, other = scratch.a, scratch.b
            x = act(cur, 0, widths[0])
            K.lpips_stem(a[g0:g1], m.w0, m.b0, normalize, out=x[:n])
            K.lpips_stem(b[g0:g1], m.w0, m.b0, normalize, out=x[n:])
            i = 0
            for k, convs in enumerate(LPIPS_STAGES):
                if k:
                    x = K.lpips_pool2(x, act(other, k, widths[k - 1]))
                    cur, other = other, cur
                for _ in range(convs - (k == 0)):
                    x = K.conv(x, m.convs[i], pad=1, act=K.ACT_RELU, prec=K.PREC_F32, out=act(other, k, widths[k]))
                    cur, other = other, cur
                    i += 1
                K.lpips_dist(x[:n], x[n:], m.lins[k], partials[first[k]:first[k] + N * strips[k]].view(N, strips[k])[g0:g1])
        return K.lpips_fold(partials, N, strips, [hk * wk for hk, wk in sizes])


def lpips_from_layers(layers) -> np.ndarray:
    """fp64 numpy [N] from layer values [N,5] (or [5] -> a 0-d array), on the host: (((d_0 + d_1) + d_2) + d_3) + d_4."""
    L = layers.detach().cpu().numpy() if isinstance(layers, torch.Tensor) else np.asarray(layers)
    L = L.astype(np.float64)
    if L.ndim not in (1, 2) or L.shape[-1] != 5:
        raise ValueError(f"layer values [N,5] expected, got {L.shape}")
    return (((L[..., 0] + L[..., 1]) + L[..., 2]) + L[..., 3]) + L[..., 4]


def lpips_u8(sr: torch.Tensor, gt: torch.Tensor, params, normalize: bool = True, scratch: LpipsScratch = None) -> np.ndarray:
    """Per-frame LPIPS (lower is better) of two uint8 [N,H,W] device stacks, result and ground truth, fp64 numpy [N] on the host:
    `lpips_layers_u8` on the device, `lpips_from_layers` on the host.  ``params``: the caller's model (`lpips_params`), checked before
    any device work; the project ships none, and parity with the ``lpips`` package is unpinned."""
    params = lpips_params(params)
    return np.atleast_1d(lpips_from_layers(lpips_layers_u8(sr, gt, params, scratch, normalize)))


def lpips_layers_u16(sr: torch.Tensor, gt: torch.Tensor, peak: int, params, scratch: LpipsScratch = None,
                     normalize: bool = True) -> torch.Tensor:
    """`lpips_layers_u8` for uint16 stacks of samples in 0 .. ``peak`` (2**depth - 1, an integer in 1 .. 65535): the stem forms
    (float)v / (float)peak, one correctly rounded fp32 division, where the 8-bit one forms (float)v / 255.f; the trunk, the distance,
    the scratch and the launches behind the stem are `lpips_layers_u8`'s.  Frames 257 k at the peak 65535 give the bits of the frames
    k."""
    peak = _metric_peak("lpips_layers_u16", peak)
    a, N, Ha, Wa, _, _ = _sample_frames(sr, "sr", torch.uint16)
    b, Nb, Hb, Wb, _, _ = _sample_frames(gt, "gt", torch.uint16)
    if N == 0 or Nb != N or a.device != b.device:
        raise ValueError(f"lpips_layers_u16: two stacks of one length on one device expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    h, w = min(Ha, Hb), min(Wa, Wb)
    sizes = lpips_size(h, w)
    params = lpips_params(params)
    widths = params.widths
    if scratch is None:
        scratch = LpipsScratch(1, h, w, widths, N, a.device)
    elif not isinstance(scratch, LpipsScratch) or scratch.device != a.device or (scratch.h, scratch.w) != (h, w) \
            or scratch.widths != widths or scratch.frames < N:
        raise ValueError(f"scratch: an lpips_scratch for at least {N} frames of a {h} x {w} region and widths {widths} on {a.device} expected")
    a, b = a[:, :h, :w], b[:, :h, :w]
    strips = scratch.strips
    with on_device(a):
        m = _lpips_on(params, a.device)
        partials = scratch.partials[:N * sum(strips)]
        first = [N * sum(strips[:k]) for k in range(5)]
        for g0 in range(0, N, scratch.pairs):
            g1 = min(g0 + scratch.pairs, N)
            n = g1 - g0
            act = lambda buf, k, c: buf[:2 * n * sizes[k][0] * sizes[k][1] * c].view(2 * n, sizes[k][0], sizes[k][1], c)
            cur, other = scratch.a, scratch.b
            x = act(cur, 0, widths[0])
            K.lpips_stem(a[g0:g1], m.w0, m.b0, normalize, out=x[:n], peak=peak)
            K.lpips_stem(b[g0:g1], m.w0, m.b0, normalize, out=x[n:], peak=peak)
            i = 0
            for k, convs in enumerate(LPIPS_STAGES):
                if k:
                    x = K.lpips_pool2(x, act(other, k, widths[k - 1]))
                    cur, other = other, cur
                for _ in range(convs - (k == 0)):
                    x = K.conv(x, m.convs[i], pad=1, act=K.ACT_RELU, prec=K.PREC_F32, out=act(other, k, widths[k]))
                    cur, other = other, cur
                    i += 1
                K.lpips_dist(x[:n], x[n:], m.lins[k], partials[first[k]:first[k] + N * strips[k]].view(N, strips[k])[g0:g1])
        return K.lpips_fold(partials, N, strips, [hk * wk for hk, wk in sizes])


def lpips_u16(sr: torch.Tensor, gt: torch.Tensor, peak: int, params, normalize: bool = True, scratch: LpipsScratch = None) -> np.ndarray:
    """`lpips_u8` for two uint16 [N,H,W] device stacks of samples in 0 .. ``peak``: `lpips_layers_u16`, then `lpips_from_layers`."""
    peak = _metric_peak("lpips_u16", peak)
    params = lpips_params(params)
    return np.atleast_1d(lpips_from_layers(lpips_layers_u16(sr, gt, peak, params, scratch, normalize)))
