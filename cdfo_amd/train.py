"""The training loop of train_LD_37.py:359-402 with nothing but the log on the host: batches come from a resident `ClipSet` (one launch
each, cdfo_amd/train_data.py), the loss is `cdfo_amd.loss.charbonnier` (one pass, no ``.item()``), forward and backward are the HIP
autograd path of ``CVSR_V8``.  The losses of an epoch stay on the device and are read once, for the reference's log line."""
from __future__ import annotations

import os
from datetime import datetime
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from .loss import charbonnier
from .train_data import ClipSet

MILESTONE, GAMMA = 2000, 0.5


def learning_rate(lr0: float, epoch: int) -> float:
    """The rate of 0-based epoch ``epoch``: ``lr0 * 0.5 ** [epoch + 1 >= 2000]``.  The reference steps its ``MultiStepLR([2000], 0.5)``
    at the TOP of each epoch (train_LD_37.py:362), so the scheduler has counted epoch + 1 steps when the epoch's batches run."""
    return lr0 * (GAMMA if epoch + 1 >= MILESTONE else 1.0)


def fit(model, clips: ClipSet, epochs: int, out_dir: str, batch_size: int = 20, crop: int = 64, lr: float = 1e-4,
        weight_decay: float = 1e-5, val_itv: int = 200, val: Optional[Sequence[str]] = None, seed: int = 4, start_epoch: int = 0,
        log: Callable[[str], None] = print, val_coding: str = "LD") -> List[float]:
    """Train ``model`` (a ``CVSR_V8`` on the clip set's device) for epochs ``start_epoch .. epochs - 1``; returns the epochs' average
    losses.  Adam with ``lr`` and ``weight_decay``; the rate of each epoch is set directly (`learning_rate`).  Every ``val_itv`` epochs
    ``state_dict()`` goes to ``<out_dir>/ckpt/epoch-N.pth`` and, with ``val = (lr_dir, side_dir, gt_dir)``, that sequence is evaluated
    (`evaluate_sequence`) and its PSNR and SSIM are logged.  ``seed`` seeds the plans' generator.  ``val_coding``: the ``coding`` of that
    evaluation ("RA": the validation flows are the random-access loader's field, what a ``ClipSet(..., coding="RA")`` trains on)."""
    from .evaluate import evaluate_sequence
    from .streaming import check_coding
    check_coding(val_coding)
    os.makedirs(os.path.join(out_dir, "ckpt"), exist_ok=True)
    rng = np.random.default_rng(seed)
    optimizer = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay)
    averages = []
    model.train()
    for epoch in range(start_epoch, epochs):
        for group in optimizer.param_groups:
            group["lr"] = learning_rate(lr, epoch)
        losses = []
        for plan in clips.epoch(batch_size, rng, crop):
            optimizer.zero_grad()
            x, mvs0, mvs1, pms, rms, ufs, hr = clips.batch(plan, crop)
            sr, _ = model(x, mvs0, mvs1, pms, rms, ufs)
            loss = charbonnier(sr, hr)
            losses.append(loss.detach())
            loss.backward()
            optimizer.step()
        per_batch = torch.stack(losses).cpu().tolist()                        # the epoch's one read of the device
        averages.append(round(sum(per_batch) / len(per_batch), 5))
        log('[%s] Epoch: %d/%d | average epoch loss: %f' % (datetime.now().strftime("%d/%m/%Y %H:%M:%S"), epoch + 1, epochs, averages[-1]))
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
