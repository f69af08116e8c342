"""The training loss on the device: the reference's Charbonnier loss (opt/loss.py:20-31), ``sum(sqrt((sr - hr)^2 + eps))``, as one HIP
pass (csrc/train_batch.hip: cdfo_charbonnier) that leaves the fp32 sum on the device and the derivative beside it -- where the script has
a six-operator torch expression and a ``loss.item()`` per step."""
from __future__ import annotations

import torch

from . import kernels as K


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
