"""The training loop of train_LD_37.py:359-402 with nothing but the log on the host: batches come from a resident `ClipSet` (one launch
each, cdfo_amd/train_data.py), the loss is `cdfo_amd.loss.charbonnier` (one pass, no ``.item()``), forward and backward are the HIP
autograd path of ``CVSR_V8``.  The losses of an epoch stay on the device and are read once, for the reference's log line.
With an LPIPS model the step's loss gains a perceptual term, `cdfo_amd.loss.lpips_loss`, the pairing opt/loss.py has with opt/lpips;
with an ``ffl_weight`` it gains a frequency term, `cdfo_amd.loss.focal_frequency_loss` (opt/deep_learning.py's Charbonnier_FFL_Loss)."""
from __future__ import annotations

import math
import os
from datetime import datetime
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from .loss import charbonnier, focal_frequency_loss, lpips_loss
from .train_data import ClipSet

MILESTONE, GAMMA = 2000, 0.5


def learning_rate(lr0: float, epoch: int) -> float:
    """The rate of 0-based epoch ``epoch``: ``lr0 * 0.5 ** [epoch + 1 >= 2000]``.  The reference steps its ``MultiStepLR([2000], 0.5)``
    at the TOP of each epoch (train_LD_37.py:362), so the scheduler has counted epoch + 1 steps when the epoch's batches run."""
    return lr0 * (GAMMA if epoch + 1 >= MILESTONE else 1.0)


def fit(model, clips: ClipSet, epochs: int, out_dir: str, batch_size: int = 20, crop: int = 64, lr: float = 1e-4,
        weight_decay: float = 1e-5, val_itv: int = 200, val: Optional[Sequence[str]] = None, seed: int = 4, start_epoch: int = 0,
        log: Callable[[str], None] = print, val_coding: str = "LD", lpips=None, lpips_weight: float = 0.0, ffl_weight: float = 0.0,
        ffl_alpha: float = 1.0) -> List[float]:
    """Train ``model`` (a ``CVSR_V8`` on the clip set's device) for epochs ``start_epoch .. epochs - 1``; returns the epochs' average
    losses.  Adam with ``lr`` and ``weight_decay``; the rate of each epoch is set directly (`learning_rate`).  Every ``val_itv`` epochs
    ``state_dict()`` goes to ``<out_dir>/ckpt/epoch-N.pth`` and, with ``val = (lr_dir, side_dir, gt_dir)``, that sequence is evaluated
    (`evaluate_sequence`) and its PSNR and SSIM are logged.  ``seed`` seeds the plans' generator.  ``val_coding``: the ``coding`` of that
    evaluation ("RA": the validation flows are the random-access loader's field, what a ``ClipSet(..., coding="RA")`` trains on).
    ``lpips``: an LPIPS model (what `metrics.lpips_params` takes); the step's loss is then ``charbonnier(sr, hr) + lpips_weight *
    lpips_loss(sr, hr, lpips).sum()``, the returned averages and the log line's loss are that total, and the line ends with
    `` | charbonnier: %f | lpips: %f``, the epoch's averages of the two terms (the second unweighted).  A model without a finite
    positive ``lpips_weight``, a weight without a model and ``crop < 4`` (the HR crop ``4 crop`` is then below LPIPS' 16 x 16) are
    ValueErrors before the first batch.  With a model two runs from one seed leave equal weights: the loss is bit-reproducible, and
    for the run `autograd.FLOW_WARP_FIXED` makes the flow warp's adjoint so.  Without a model every result, log line, allocation and
    launch is what it was.
    ``ffl_weight``: a finite positive weight adds ``ffl_weight * focal_frequency_loss(sr, hr, ffl_alpha).sum()`` to the step's loss
    (after the LPIPS term when both are on); averages and the logged loss are the total, and the line ends with `` | charbonnier: %f``
    ``[ | lpips: %f]`` `` | ffl: %f`` (unweighted).  The run is reproducible as the LPIPS run is (`autograd.FLOW_WARP_FIXED`).  A
    negative, non-finite or bool weight, an ``ffl_alpha`` other than 1.0 without a weight (or one that is not a finite number >= 0)
    and a ``crop`` that is not a power of two from 4 to 128 (the HR crop is the transform's size) are ValueErrors before the first
    batch.  With ``ffl_weight = 0.0`` nothing changes."""
    from .streaming import check_coding
    check_coding(val_coding)
    if lpips is None:
        if lpips_weight:
            raise ValueError(f"fit: lpips_weight {lpips_weight!r} needs an LPIPS model (lpips=)")
    else:
        from .metrics import lpips_params
        if isinstance(lpips_weight, bool) or not isinstance(lpips_weight, (int, float)) or not math.isfinite(lpips_weight) or lpips_weight <= 0:
            raise ValueError(f"fit: an LPIPS model needs a finite positive lpips_weight, got {lpips_weight!r}")
        if crop < 4:
            raise ValueError(f"fit: LPIPS needs an HR crop of at least 16 x 16, got crop = {crop} (HR {4 * crop} x {4 * crop})")
        lpips = lpips_params(lpips)
    if isinstance(ffl_weight, bool) or not isinstance(ffl_weight, (int, float)) or not math.isfinite(ffl_weight) or ffl_weight < 0:
        raise ValueError(f"fit: ffl_weight must be a finite number >= 0, got {ffl_weight!r}")
    if ffl_weight:
        from .kernels import ffl_alpha as check_alpha
        ffl_alpha = check_alpha(ffl_alpha, "fit: ffl_alpha")
        if isinstance(crop, bool) or not isinstance(crop, int) or not 4 <= crop <= 128 or crop & (crop - 1):
            raise ValueError(f"fit: ffl_weight needs a crop that is a power of two from 4 to 128 (HR 16 .. 512), got crop = {crop!r}")
    elif isinstance(ffl_alpha, bool) or ffl_alpha != 1.0:
        raise ValueError(f"fit: ffl_alpha {ffl_alpha!r} needs an ffl_weight")
    if lpips is not None or ffl_weight:    # two runs from one seed then leave equal weights: the warp's adjoint adds in a fixed-point order
        from . import autograd
        was, autograd.FLOW_WARP_FIXED = autograd.FLOW_WARP_FIXED, True
        try:
            return _fit(model, clips, epochs, out_dir, batch_size, crop, lr, weight_decay, val_itv, val, seed, start_epoch, log, val_coding,
                        lpips, lpips_weight, float(ffl_weight), ffl_alpha)
        finally:
            autograd.FLOW_WARP_FIXED = was
    return _fit(model, clips, epochs, out_dir, batch_size, crop, lr, weight_decay, val_itv, val, seed, start_epoch, log, val_coding, None, 0.0)


def _fit(model, clips, epochs, out_dir, batch_size, crop, lr, weight_decay, val_itv, val, seed, start_epoch, log, val_coding, lpips,
         lpips_weight, ffl_weight=0.0, ffl_alpha=1.0) -> List[float]:
    """The loop of `fit` behind its argument checks."""
    from .evaluate import evaluate_sequence
    os.makedirs(os.path.join(out_dir, "ckpt"), exist_ok=True)
    rng = np.random.default_rng(seed)
    optimizer = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay)
    averages = []
    model.train()
    for epoch in range(start_epoch, epochs):
        for group in optimizer.param_groups:
            group["lr"] = learning_rate(lr, epoch)
        losses, terms = [], []
        for plan in clips.epoch(batch_size, rng, crop):
            optimizer.zero_grad()
            x, mvs0, mvs1, pms, rms, ufs, hr = clips.batch(plan, crop)
            sr, _ = model(x, mvs0, mvs1, pms, rms, ufs)
            loss = charbonnier(sr, hr)
            if lpips is not None or ffl_weight:
                parts = [loss.detach()]
                if lpips is not None:
                    perc = lpips_loss(sr, hr, lpips).sum()
                    loss = loss + lpips_weight * perc
                    parts.append(perc.detach())
                if ffl_weight:
                    freq = focal_frequency_loss(sr, hr, ffl_alpha).sum()
                    loss = loss + ffl_weight * freq
                    parts.append(freq.detach())
                terms.append(torch.stack(parts))
            losses.append(loss.detach())
            loss.backward()
            optimizer.step()
        per_batch = torch.stack(losses).cpu().tolist()                        # the epoch's one read of the device
        averages.append(round(sum(per_batch) / len(per_batch), 5))
        line = '[%s] Epoch: %d/%d | average epoch loss: %f' % (datetime.now().strftime("%d/%m/%Y %H:%M:%S"), epoch + 1, epochs, averages[-1])
        if terms:
            names = ['charbonnier'] + ['lpips'] * (lpips is not None) + ['ffl'] * bool(ffl_weight)
            line += ''.join(' | %s: %f' % nv for nv in zip(names, torch.stack(terms).mean(dim=0).cpu().tolist()))
        log(line)
        if (epoch + 1) % val_itv == 0:
            torch.save(model.state_dict(), os.path.join(out_dir, "ckpt", "epoch-%d.pth" % (epoch + 1)))
            log('Saved model. lr %f' % optimizer.param_groups[0]["lr"])
            if val is not None:
                model.eval()
                with torch.no_grad():
                    r = evaluate_sequence(model, val[0], val[1], gt_dir=val[2], coding=val_coding)
                model.train()
                log('PSNR:%f, SSIM: %f' % (r.mean_psnr, r.mean_ssim))
    return averages
