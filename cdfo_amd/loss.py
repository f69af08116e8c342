"""The training loss on the device: the reference's Charbonnier loss (opt/loss.py:20-31), ``sum(sqrt((sr - hr)^2 + eps))``, as one HIP
pass (csrc/train_batch.hip: cdfo_charbonnier) that leaves the fp32 sum on the device and the derivative beside it -- where the script has
a six-operator torch expression and a ``loss.item()`` per step.

`lpips_loss` is the perceptual distance the evaluators score with (`cdfo_amd.metrics.lpips_u8`) as a training loss, the pairing of the
reference's opt/loss.py with opt/lpips: the metric's launches behind a float stem, and an explicit backward through the frozen trunk
on the device (csrc/lpips.hip).

`focal_frequency_loss` is the frequency term of the reference's ``Focal_Frequecny_Loss`` / ``Charbonnier_FFL_Loss``
(opt/deep_learning.py:192-220), by the project's own definition written after the defaults of the package those classes call: a 2-D
FFT in HIP, the spectrum weighted by its own magnitude, and the inverse FFT for the gradient (csrc/ffl.hip).

`ssim_loss` and `msssim_loss` are ``1 - SSIM`` and ``1 - MS-SSIM`` by the definitions the evaluators score with
(`cdfo_amd.metrics.calculate_ssim`, `msssim_u8`) on float frames, with the exact gradient: the window as two separable passes through
LDS in fp64, forward and adjoint (csrc/ssim_loss.hip)."""
from __future__ import annotations

import torch

from . import kernels as K
from . import metrics as M


class _Charbonnier(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sr, hr, eps):
        with K.on_device(sr):
            loss, g = K.charbonnier(sr.detach(), hr.detach(), eps)
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (g,) = ctx.saved_tensors
        return grad_out * g, None, None


def charbonnier(sr: torch.Tensor, hr: torch.Tensor, eps: float = 1e-4) -> torch.Tensor:
    """fp32 scalar on the device.  ``sr`` and ``hr``: dense fp32 device tensors of one shape (anything else is a ValueError; nothing is
    made contiguous or cast behind the caller's back).  The terms are accumulated in fp64 in a fixed order: equal inputs give equal
    bits.  Backward is ``grad_out * (sr - hr) / sqrt((sr - hr)^2 + eps)`` for ``sr`` and none for ``hr``.  Non-finite inputs
    propagate; nothing is clamped; there is no host synchronisation."""
    if not sr.is_cuda:
        raise NotImplementedError("charbonnier: the HIP path needs device tensors (there is no CPU fallback)")
    return _Charbonnier.apply(sr, hr, float(eps))


class _Lpips(torch.autograd.Function):
    """The forward is `metrics.lpips_layers_f32`'s launches on all N pairs as one batch, with the result's thirteen activations and
    the ground truth's five taps copied out of the ping-pong scratch; the backward walks the stages 5 -> 1."""

    @staticmethod
    def forward(ctx, sr, hr, params, normalize):
        a, b = sr.detach().view(sr.shape[0], sr.shape[-2], sr.shape[-1]), hr.detach().view(hr.shape[0], hr.shape[-2], hr.shape[-1])
        N, h, w = a.shape
        acts, taps = [None] * M.LPIPS_CONVS, []
        last = [sum(M.LPIPS_STAGES[:k + 1]) - 1 for k in range(5)]

        def keep(i, x, n):
            acts[i] = x[:n].clone()
            if i in last:
                taps.append(x[n:].clone())

        with K.on_device(a):
            scratch = M.LpipsScratch(N, h, w, params.widths, N, a.device)
            layers = M._lpips_layers_f32(a, b, params, scratch, normalize, keep)
            loss = ((((layers[:, 0] + layers[:, 1]) + layers[:, 2]) + layers[:, 3]) + layers[:, 4]).float()
        ctx.params, ctx.normalize, ctx.shape = params, normalize, sr.shape
        ctx.save_for_backward(*acts, *taps)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        from .autograd import act_bwd
        saved = ctx.saved_tensors
        acts, taps = saved[:M.LPIPS_CONVS], saved[M.LPIPS_CONVS:]
        gscale = grad_out.detach().to(torch.float32).contiguous()
        with K.on_device(gscale):
            m = M._lpips_adjoint_on(ctx.params, gscale.device)
            gin, i = None, M.LPIPS_CONVS - 1
            for k in range(4, -1, -1):
                g = K.lpips_dist_bwd(acts[i], taps[k], m.lins[k], gscale, gin)       # at conv i's pre-activation
                for _ in range(M.LPIPS_STAGES[k] - 1):
                    g = K.conv(g, m.adj[i - 1], pad=1, prec=K.PREC_F32)               # at conv i - 1's output ...
                    i -= 1
                    g = act_bwd(g, acts[i], K.ACT_RELU)                               # ... and through its ReLU
                if k:
                    g = K.conv(g, m.adj[i - 1], pad=1, prec=K.PREC_F32)               # at the pool's output
                    i -= 1
                    gin = K.lpips_pool2_bwd(acts[i], g)                               # at the tap before, in front of its select
            gx = K.lpips_stem_bwd(g, m.wf[ctx.normalize])
        return gx.view(ctx.shape), None, None, None


def lpips_loss(sr: torch.Tensor, hr: torch.Tensor, model, normalize: bool = True) -> torch.Tensor:
    """Per-frame LPIPS of ``sr`` to ``hr`` as a loss: fp32 [N] on the device, the fp64 total (((d0 + d1) + d2) + d3) + d4 of
    `metrics.lpips_layers_f32` rounded once.  ``sr``, ``hr``: dense fp32 device tensors [N,1,H,W] or [N,H,W] of one shape, H, W >= 16,
    samples nominally in 0 .. 1 and used as they are (no / 255, no clamp, no quantisation); anything else is a ValueError, nothing is
    made contiguous or cast.  ``model``: what `metrics.lpips_params` takes, checked before any device work; its weights are frozen.
    Gradient flows to ``sr`` only (``hr`` gets None), through the fp32 trunk by explicit HIP adjoints; a ReLU output <= 0 passes +0
    whatever arrives (a select), a max-pool routes to the element ATen's CPU kernel picks.  Equal inputs give equal bits, forward and
    backward; ``sr`` equal to ``hr`` gives exactly 0 and an all-zero gradient.  There is no host synchronisation.

    Kept between forward and backward, in bytes: ``4 N sum_k h_k w_k C_k (convs_k + 1)`` with (h_k, w_k) = (H >> k, W >> k), C_k the
    stage widths and convs = (2, 2, 3, 3, 3) -- the result's thirteen activations and the ground truth's five taps.  The forward also
    holds, until it returns, two ping-pong buffers of ``8 N max_k h_k w_k C_k`` bytes each."""
    params = M.lpips_params(model)
    a, b = M._lpips_f32_frames(sr, "lpips_loss: sr"), M._lpips_f32_frames(hr, "lpips_loss: hr")
    if sr.shape != hr.shape or sr.device != hr.device:
        raise ValueError(f"lpips_loss: two tensors of one shape on one device expected, got {tuple(sr.shape)} and {tuple(hr.shape)}")
    M.lpips_size(a.shape[1], a.shape[2])
    return _Lpips.apply(sr, hr, params, bool(normalize))


class _FocalFrequency(torch.autograd.Function):
    """As `_Charbonnier`: the forward leaves the derivative beside the loss.  Entered only when ``sr`` needs a gradient."""

    @staticmethod
    def forward(ctx, sr, hr, alpha):
        with K.on_device(sr):
            loss, g = K.ffl_loss(sr.detach(), hr.detach(), alpha, want_grad=True)
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (g,) = ctx.saved_tensors
        return grad_out.view(-1, *([1] * (g.dim() - 1))) * g, None, None


def focal_frequency_loss(sr: torch.Tensor, hr: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
    """Per-frame focal frequency loss of ``sr`` to ``hr``: fp32 [N] on the device.  The project's own definition, after the defaults
    of the ``focal_frequency_loss`` package (patch_factor 1, no averaged spectrum, no log or batch matrix); parity with the package is
    not pinned.  For a frame of H x W samples: ``d = sr - hr`` (one fp32 subtraction; the transform is linear, so the package's
    difference of two spectra is this in exact arithmetic), ``F = fft2(d, norm="ortho")``, ``D = Re(F)^2 + Im(F)^2``,
    ``M = sqrt(D) ** alpha`` (0 ** 0 = 1), ``w = M / max(M)`` over the frame's bins, NaN -> 0, clamped to [0, 1] and held constant for
    the gradient, ``loss = sum(w D) / (H W)``.  ``alpha = 0`` weighs every bin 1: the loss is mean(d^2).

    ``sr``, ``hr``: dense fp32 device tensors [N,1,H,W] or [N,H,W] of one shape on one device, H and W powers of two from 16 to 512
    (they may differ); ``alpha`` a finite number >= 0 (the kernels take it as fp32).  Anything else is a ValueError before any device
    work; nothing is made contiguous or cast; CPU tensors raise NotImplementedError.  Gradient flows to ``sr`` only (``hr`` gets
    None) and is exact, ``2 / (H W) Re(ifft2(w F, norm="ortho"))``, scaled by the upstream gradient of the frame.  The weights, the
    terms and their sum are fp64 in a fixed order and nothing is atomic: equal inputs give equal bits, forward and backward; ``sr``
    equal to ``hr`` gives exactly 0 and an all-zero gradient.  A frame with a non-finite sample gets a NaN loss and an unspecified
    gradient; the other frames are untouched.  There is no host synchronisation.

    Kept between forward and backward: the gradient, ``4 N H W`` bytes (nothing under ``no_grad`` or when ``sr`` needs no gradient:
    the inverse passes are then not launched).  The forward also holds, until it returns, the spectrum (``8 N H W`` bytes) and two
    fp64 arrays of ``N W / 16`` (``N W / 8`` at H = 512) and ``N max(1, H W / 4096)`` values."""
    if not sr.is_cuda or not hr.is_cuda:
        raise NotImplementedError("focal_frequency_loss: the HIP path needs device tensors (there is no CPU fallback)")
    K._ffl_frames(sr, hr, "focal_frequency_loss")
    alpha = K.ffl_alpha(alpha, "focal_frequency_loss")
    if not (torch.is_grad_enabled() and sr.requires_grad):                  # hr gets no gradient: nothing to record
        with K.on_device(sr):
            return K.ffl_loss(sr.detach(), hr.detach(), alpha, want_grad=False)[0]
    return _FocalFrequency.apply(sr, hr, alpha)


class _StructuralLoss(torch.autograd.Function):
    """As `_FocalFrequency`: the forward leaves the derivative beside the loss.  Entered only when ``sr`` needs a gradient."""

    @staticmethod
    def forward(ctx, sr, hr, peak, levels):
        with K.on_device(sr):
            loss, g = K.ssim_loss(sr.detach(), hr.detach(), peak, levels, want_grad=True)
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (g,) = ctx.saved_tensors
        return grad_out.view(-1, *([1] * (g.dim() - 1))) * g, None, None, None


def _structural_loss(sr, hr, peak, levels, who):
    if not sr.is_cuda or not hr.is_cuda:
        raise NotImplementedError(f"{who}: the HIP path needs device tensors (there is no CPU fallback)")
    K._ssim_loss_frames(sr, hr, levels, who)
    peak = K.ssim_loss_peak(peak, who)
    if not (torch.is_grad_enabled() and sr.requires_grad):                  # hr gets no gradient: nothing to record
        with K.on_device(sr):
            return K.ssim_loss(sr.detach(), hr.detach(), peak, levels, want_grad=False)[0]
    return _StructuralLoss.apply(sr, hr, peak, levels)


def ssim_loss(sr: torch.Tensor, hr: torch.Tensor, peak: float = 1.0) -> torch.Tensor:
    """Per-frame ``1 - SSIM`` of ``sr`` to ``hr``: fp32 [N] on the device, by the project's own definition (the metric's,
    `metrics.calculate_ssim` with ``crop_border=0, from_unit_range=False`` at ``peak = 255``).  Samples are used as they are: no scale,
    no clamp, no quantisation, no crop border.  With the separable 11-tap Gaussian G of sigma 1.5 over valid positions only,
    ``C1 = (0.01 peak)^2``, ``C2 = (0.03 peak)^2``, and everything behind the fp32 loads in fp64: ``m1 = G*sr``, ``m2 = G*hr``,
    ``e11 = G*sr^2``, ``e22 = G*hr^2``, ``e12 = G*(sr hr)``, ``cs = (2 (e12 - m1 m2) + C2) / ((e11 - m1^2) + (e22 - m2^2) + C2)``,
    ``l = (2 m1 m2 + C1) / (m1^2 + m2^2 + C1)``, ``loss = 1 - mean(l cs)`` over the (H - 10)(W - 10) positions.

    ``sr``, ``hr``: dense fp32 device tensors [N,1,H,W] or [N,H,W] of one shape on one device, H, W >= 11; ``peak`` a finite number
    > 0.  Anything else is a ValueError before any device work; nothing is made contiguous or cast; CPU tensors raise
    NotImplementedError.  Gradient flows to ``sr`` only (``hr`` gets None) and is exact: ``Gt*P + 2 sr Gt*Q + hr Gt*R`` with P, Q, R
    the derivatives of the mean by m1, e11, e12 and ``Gt*`` the full correlation, scaled by the upstream gradient of the frame.  Sums
    run in a fixed order and nothing is atomic: equal inputs give equal bits, forward and backward.  The loss is rounded to fp32 once
    and so is every gradient element.  There is no host synchronisation.

    Kept between forward and backward: the gradient, ``4 N H W`` bytes (nothing under ``no_grad`` or when ``sr`` needs no gradient:
    the gradient passes are then not launched).  The forward also holds, until it returns, the tile sums, means and coefficients (fp64,
    ``N (2 T + 4)`` values for T tiles of 16 x 32 positions) and, for the gradient, three fp64 maps, ``24 N (H - 10)(W - 10)`` bytes."""
    return _structural_loss(sr, hr, peak, 1, "ssim_loss")


def msssim_loss(sr: torch.Tensor, hr: torch.Tensor, peak: float = 1.0) -> torch.Tensor:
    """Per-frame ``1 - MS-SSIM`` of ``sr`` to ``hr`` over five scales: fp32 [N] on the device, by the project's own definition
    (`metrics.msssim_u8`'s on float frames).  Level j + 1 is the 2 x 2 non-overlapping mean of level j from the top-left
    sample, a trailing odd row or column dropped, held in fp32: a sample is ``fp32(((a + b) + c) + d in fp64, times 0.25)``.  With
    `ssim_loss`'s cs and l per level, ``M_cs[j] = mean(cs)``, ``M_ssim[j] = mean(l cs)`` and `metrics.MSSSIM_WEIGHTS` w:
    ``loss = 1 - prod_{j<4} max(M_cs[j], 0)^w[j] max(M_ssim[4], 0)^w[4]``.  If any of those five means is <= 0 the loss is exactly 1 and
    the frame's gradient exactly zero.

    Arguments, errors and reproducibility as `ssim_loss`, with ``min(H, W) >= metrics.msssim_min_size`` (176).  The gradient is exact
    with the pool's rounding taken as the identity: a coarser level's gradient reaches each of a sample's four parents as a quarter of
    its value, a dropped row or column gets none; levels above 0 keep theirs in fp64, so an element is rounded once.

    Kept between forward and backward: the gradient, ``4 N H W`` bytes (nothing when none is wanted).  The forward also holds, until it
    returns, levels 1 .. 4 of both frames (``8 N sum_j h_j w_j`` bytes, about ``2.7 N H W``), the tile sums, means and coefficients,
    and for the gradient three fp64 maps of level 0's size (``24 N (H - 10)(W - 10)`` bytes) and up to two fp64 level gradients
    (``8 N h_j w_j`` bytes each, j >= 1)."""
    return _structural_loss(sr, hr, peak, 5, "msssim_loss")
