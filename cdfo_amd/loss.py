"""The training loss on the device: the reference's Charbonnier loss (opt/loss.py:20-31), ``sum(sqrt((sr - hr)^2 + eps))``, as one HIP
pass (csrc/train_batch.hip: cdfo_charbonnier) that leaves the fp32 sum on the device and the derivative beside it -- where the script has
a six-operator torch expression and a ``loss.item()`` per step.

`lpips_loss` is the perceptual distance the evaluators score with (`cdfo_amd.metrics.lpips_u8`) as a training loss, the pairing of the
reference's opt/loss.py with opt/lpips: the metric's launches behind a float stem, and an explicit backward through the frozen trunk
on the device (csrc/lpips.hip).

`focal_frequency_loss` is the frequency term of the reference's ``Focal_Frequecny_Loss`` / ``Charbonnier_FFL_Loss``
(opt/deep_learning.py:192-220), by the project's own definition written after the defaults of the package those classes call: a 2-D
FFT in HIP, the spectrum weighted by its own magnitude, and the inverse FFT for the gradient (csrc/ffl.hip)."""
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
