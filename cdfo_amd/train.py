"""The training loop of train_LD_37.py:359-402 with nothing but the log on the host: batches come from a resident `ClipSet` (one launch
each, cdfo_amd/train_data.py), the loss is `cdfo_amd.loss.charbonnier` (one pass, no ``.item()``), forward and backward are the HIP
autograd path of ``CVSR_V8``.  The losses of an epoch stay on the device and are read once, for the reference's log line.
With an LPIPS model the step's loss gains a perceptual term, `cdfo_amd.loss.lpips_loss`, the pairing opt/loss.py has with opt/lpips;
with an ``ffl_weight`` it gains a frequency term, `cdfo_amd.loss.focal_frequency_loss` (opt/deep_learning.py's Charbonnier_FFL_Loss);
with an ``ssim_weight`` a structural one, `cdfo_amd.loss.ssim_loss` or `msssim_loss`, the figures the evaluators score with."""
from __future__ import annotations

import contextlib
import copy
import math
import os
from datetime import datetime
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from .loss import charbonnier, focal_frequency_loss, lpips_loss, msssim_loss, ssim_loss
from .train_data import ClipSet

MILESTONE, GAMMA = 2000, 0.5


def learning_rate(lr0: float, epoch: int) -> float:
    """The rate of 0-based epoch ``epoch``: ``lr0 * 0.5 ** [epoch + 1 >= 2000]``.  The reference steps its ``MultiStepLR([2000], 0.5)``
    at the TOP of each epoch (train_LD_37.py:362), so the scheduler has counted epoch + 1 steps when the epoch's batches run."""
    return lr0 * (GAMMA if epoch + 1 >= MILESTONE else 1.0)


def fit(model, clips: ClipSet, epochs: int, out_dir: str, batch_size: int = 20, crop: int = 64, lr: float = 1e-4,
        weight_decay: float = 1e-5, val_itv: int = 200, val: Optional[Sequence[str]] = None, seed: int = 4, start_epoch: int = 0,
        log: Callable[[str], None] = print, val_coding: str = "LD", lpips=None, lpips_weight: float = 0.0, ffl_weight: float = 0.0,
        ffl_alpha: float = 1.0, optimizer: str = "torch", max_grad_norm: Optional[float] = None, deterministic: bool = False,
        save_state: bool = False, resume: Optional[str] = None, ssim_weight: float = 0.0, ssim_scales: int = 1) -> List[float]:
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
    batch.  With ``ffl_weight = 0.0`` nothing changes.
    ``optimizer``: "torch" (``torch.optim.Adam``) or "device" (`cdfo_amd.optim.DeviceAdam` with the same hyper-parameters: three
    launches a step, a step with a non-finite gradient is skipped instead of ending the run).  With "device" the epoch's line ends with
    `` | grad norm: %f``, the mean norm before clipping over the epoch's unskipped steps, and `` | skipped: %d`` when the epoch
    skipped steps; both come with the losses in the epoch's one read.  ``max_grad_norm``: a finite positive number clips the
    gradient to that norm (``clip_grad_norm_``'s coefficient) and needs ``optimizer="device"``.  ``deterministic``: sets
    `autograd.FLOW_WARP_FIXED` for the run, as an LPIPS or FFL term does.  ``save_state``: beside every ``epoch-N.pth`` (unchanged)
    goes ``epoch-N.state.pth``: the optimizer's state dict and kind, the epoch, the averages so far, the states of the plans'
    generator and of torch's CPU and device generators, and the run-defining arguments (`RUN_ARGUMENTS`); plain tensors and Python
    values, written after the checkpoint's validation.  ``resume``: such a file; the weights come from its sibling ``epoch-N.pth``,
    everything above is restored and the run continues at epoch N (``start_epoch`` stays 0), bit for bit when the run is
    reproducible (``deterministic`` or a loss term that sets it).  A state of either optimizer continues on the other.  A state file
    whose run-defining arguments differ from the call's (the first difference is named), a missing sibling and ``epochs <= N`` are
    ValueErrors before the first batch.  Without these keywords nothing changes.
    ``ssim_weight``: a finite positive weight adds ``ssim_weight * ssim_loss(sr, hr).sum()`` (``ssim_scales = 1``) or ``ssim_weight *
    msssim_loss(sr, hr).sum()`` (``ssim_scales = 5``) to the step's loss, after the FFL term when both are on; averages and the logged
    loss are the total, and the line gains `` | ssim: %f`` or `` | msssim: %f`` (unweighted) behind the other terms.  The run is
    reproducible as the LPIPS run is (`autograd.FLOW_WARP_FIXED`).  A negative, non-finite or bool weight, ``ssim_scales`` outside
    {1, 5}, five scales without a weight, ``crop < 3`` for one scale (the HR crop ``4 crop`` is then below the 11-tap window) and
    ``crop < 44`` for five (below `metrics.msssim_min_size`) are ValueErrors before the first batch.  A state file written before
    these keywords existed reads as ``ssim_weight = 0.0, ssim_scales = 1``.  With ``ssim_weight = 0.0`` nothing changes."""
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
    if isinstance(ssim_weight, bool) or not isinstance(ssim_weight, (int, float)) or not math.isfinite(ssim_weight) or ssim_weight < 0:
        raise ValueError(f"fit: ssim_weight must be a finite number >= 0, got {ssim_weight!r}")
    if isinstance(ssim_scales, bool) or ssim_scales not in (1, 5):
        raise ValueError(f"fit: ssim_scales must be 1 or 5, got {ssim_scales!r}")
    if ssim_weight:
        need = 3 if ssim_scales == 1 else 44
        if isinstance(crop, bool) or not isinstance(crop, int) or crop < need:
            raise ValueError(f"fit: ssim_weight with ssim_scales = {ssim_scales} needs crop >= {need} (an HR crop of at least "
                             f"{11 if ssim_scales == 1 else 176} samples each way), got crop = {crop!r}")
    elif ssim_scales != 1:
        raise ValueError(f"fit: ssim_scales {ssim_scales!r} needs an ssim_weight")
    ssim_scales = int(ssim_scales)
    if optimizer not in ("torch", "device"):
        raise ValueError(f"fit: optimizer must be 'torch' or 'device', got {optimizer!r}")
    if max_grad_norm is not None:
        from .optim import _check_max_norm
        max_grad_norm = _check_max_norm(max_grad_norm, "fit")
        if optimizer != "device":
            raise ValueError("fit: max_grad_norm needs optimizer='device'")
    if not lpips_weight:
        lpips_weight = 0.0
    run = run_arguments(batch_size, crop, lr, weight_decay, seed, clips.coding, lpips_weight, float(ffl_weight), ffl_alpha, max_grad_norm,
                        ssim_weight=float(ssim_weight), ssim_scales=ssim_scales)
    state = None
    if resume is not None:
        if start_epoch != 0:
            raise ValueError(f"fit: resume continues at the state file's epoch; start_epoch must stay 0, got {start_epoch!r}")
        state = read_state(resume, run, epochs)
    # two runs from one seed then leave equal weights: the warp's adjoint adds in a fixed-point order
    with _flow_warp_fixed(bool(deterministic) or lpips is not None or bool(ffl_weight) or bool(ssim_weight)):
        return _fit(model, clips, epochs, out_dir, batch_size, crop, lr, weight_decay, val_itv, val, seed, start_epoch, log, val_coding,
                    lpips, lpips_weight, float(ffl_weight), ffl_alpha, optimizer, max_grad_norm, bool(save_state), state, run,
                    float(ssim_weight), ssim_scales)


@contextlib.contextmanager
def _flow_warp_fixed(on: bool):
    """`autograd.FLOW_WARP_FIXED` set for the block when ``on``: the one place a run is made reproducible."""
    if not on:
        yield
        return
    from . import autograd
    was, autograd.FLOW_WARP_FIXED = autograd.FLOW_WARP_FIXED, True
    try:
        yield
    finally:
        autograd.FLOW_WARP_FIXED = was


# ---- the state file: what a run needs, beside its weights, to continue bit for bit -------------------------------------------------

RUN_ARGUMENTS = ("batch_size", "crop", "lr", "weight_decay", "seed", "coding", "lpips_weight", "ffl_weight", "ffl_alpha", "max_grad_norm",
                 "ssim_weight", "ssim_scales")


def run_arguments(batch_size, crop, lr, weight_decay, seed, coding, lpips_weight, ffl_weight, ffl_alpha, max_grad_norm,
                  ssim_weight=0.0, ssim_scales=1) -> dict:
    """The arguments that define a run, as the state file keeps them (`RUN_ARGUMENTS`' order)."""
    return dict(zip(RUN_ARGUMENTS, (batch_size, crop, lr, weight_decay, seed, coding, lpips_weight, ffl_weight, ffl_alpha, max_grad_norm,
                                    ssim_weight, ssim_scales)))


_ARGUMENT_DEFAULTS = {"ssim_weight": 0.0, "ssim_scales": 1}       # names a state file written before they existed does not record


def check_run_arguments(saved: dict, current: dict, path: str = "the state file") -> None:
    """ValueError naming the first of `RUN_ARGUMENTS` in which the state file's run differs from the call's.  A file that lacks
    ``ssim_weight`` / ``ssim_scales`` was written by a run without the term: they read as 0.0 and 1."""
    for name in RUN_ARGUMENTS:
        if name not in saved and name not in _ARGUMENT_DEFAULTS:
            raise ValueError(f"fit: {path} does not record {name}")
        was = saved[name] if name in saved else _ARGUMENT_DEFAULTS[name]
        if was != current[name] or (was is None) != (current[name] is None):
            raise ValueError(f"fit: {path} was written by a run with {name} = {was!r}, this call has {name} = {current[name]!r}")


def _plain(x):
    """Tensors on the CPU, containers and Python values as they are: what ``torch.load`` reads with its defaults."""
    if isinstance(x, torch.Tensor):
        return x.detach().cpu()
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_plain(v) for v in x)
    if isinstance(x, np.generic):
        return x.item()
    return x


def generator_states(rng: np.random.Generator, device=None) -> dict:
    """The state of the plans' generator, of torch's CPU generator and of torch's generator of ``device`` (the Gumbel keys' source)."""
    cuda = device is not None and torch.device(device).type == "cuda"
    return {"numpy": _plain(copy.deepcopy(rng.bit_generator.state)), "torch_cpu": torch.get_rng_state().clone(),
            "torch_device": torch.cuda.get_rng_state(device).clone() if cuda else None}


def set_generator_states(rng: np.random.Generator, states: dict, device=None) -> None:
    """Put `generator_states` back: the next draws are those that followed the call that took them."""
    if states["numpy"]["bit_generator"] != rng.bit_generator.state["bit_generator"]:
        raise ValueError(f"fit: the state file's plan generator is a {states['numpy']['bit_generator']}, this run's a "
                         f"{rng.bit_generator.state['bit_generator']}")
    rng.bit_generator.state = states["numpy"]
    torch.set_rng_state(states["torch_cpu"].cpu())
    if states.get("torch_device") is not None and device is not None and torch.device(device).type == "cuda":
        torch.cuda.set_rng_state(states["torch_device"].cpu(), device)


def state_path(out_dir: str, epoch: int) -> str:
    return os.path.join(out_dir, "ckpt", "epoch-%d.state.pth" % epoch)


def weights_beside(path: str) -> str:
    """``.../epoch-N.pth`` for the state file ``.../epoch-N.state.pth``."""
    if not path.endswith(".state.pth"):
        raise ValueError(f"fit: resume takes a state file (epoch-N.state.pth), got {path!r}")
    return path[:-len(".state.pth")] + ".pth"


def write_state(path: str, optimizer, kind: str, epoch: int, averages, rng, device, run: dict) -> None:
    """A run without a structural term writes the file it always wrote: a name of `_ARGUMENT_DEFAULTS` at its default is left out
    (`check_run_arguments` reads its absence as that default)."""
    opt = optimizer.state_dict()
    run = {k: v for k, v in run.items() if k not in _ARGUMENT_DEFAULTS or v != _ARGUMENT_DEFAULTS[k]}
    torch.save({"optimizer": _plain(opt), "optimizer_kind": kind, "epoch": int(epoch), "averages": [float(a) for a in averages],
                "generators": generator_states(rng, device), "run": _plain(dict(run))}, path)


def read_state(path: str, run: dict, epochs: int) -> dict:
    """The state file at ``path``, checked against the call: its run-defining arguments, its sibling weights, its epoch."""
    if not os.path.isfile(path):
        raise ValueError(f"fit: no state file at {path!r}")
    weights = weights_beside(path)
    state = torch.load(path, map_location="cpu")
    for key in ("optimizer", "optimizer_kind", "epoch", "averages", "generators", "run"):
        if not isinstance(state, dict) or key not in state:
            raise ValueError(f"fit: {path!r} is not a state file: no {key!r}")
    check_run_arguments(state["run"], run, repr(path))
    if not os.path.isfile(weights):
        raise ValueError(f"fit: the weights of {path!r} are missing: no {weights!r}")
    if epochs <= state["epoch"]:
        raise ValueError(f"fit: {path!r} is the state after epoch {state['epoch']}; epochs = {epochs!r} leaves nothing to run")
    state["weights"] = weights
    return state


def _adam_state_by_name(opt_state: dict, all_names: List[str]):
    """An optimizer state of either kind as a `DeviceAdam.state_dict()` whose ``names`` say which parameters the moments belong to;
    None for a torch state that holds no moments yet."""
    from .optim import adam_moments
    if "param_groups" not in opt_state:
        if opt_state.get("names") is None:
            raise ValueError("fit: the state file's optimizer state does not name its parameters")
        return opt_state
    indices = sorted(opt_state["state"])
    if not indices:
        return None
    if len(opt_state["param_groups"]) != 1 or len(opt_state["param_groups"][0]["params"]) != len(all_names):
        raise ValueError("fit: the state file's optimizer state is not over this model's parameters")
    step, skipped, m, v, _ = adam_moments(opt_state, len(indices), indices)
    return {"step": step, "skipped": skipped, "names": [all_names[i] for i in indices], "exp_avg": m, "exp_avg_sq": v}


def _fit(model, clips, epochs, out_dir, batch_size, crop, lr, weight_decay, val_itv, val, seed, start_epoch, log, val_coding, lpips,
         lpips_weight, ffl_weight=0.0, ffl_alpha=1.0, kind="torch", max_grad_norm=None, save_state=False, state=None, run=None,
         ssim_weight=0.0, ssim_scales=1) -> List[float]:
    """The loop of `fit` behind its argument checks."""
    from .evaluate import evaluate_sequence
    os.makedirs(os.path.join(out_dir, "ckpt"), exist_ok=True)
    rng = np.random.default_rng(seed)
    on_device = kind == "device"
    named = dict(model.named_parameters())

    def device_adam(names):
        from .optim import DeviceAdam
        return DeviceAdam([(n, named[n]) for n in names], lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm)

    # DeviceAdam wants a gradient for every parameter it was given; the model has parameters no loss reaches (torch.optim.Adam passes
    # them by).  So it is made over the parameters that have a gradient after the first backward, or over those the state file names.
    optimizer = None if on_device else torch.optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay)
    if on_device:                                # what the torch path's first zero_grad() does: a stale .grad is not the first step's
        for p in named.values():
            p.grad = None
    averages = []
    device = next(model.parameters()).device
    seen = (0, 0, 0.0)                           # DeviceAdam's (step, skipped, sum of norms) at the top of the epoch
    if state is not None:
        model.load_state_dict(torch.load(state["weights"], map_location=device))
        saved = _adam_state_by_name(state["optimizer"], list(named))
        if on_device and saved is not None:
            optimizer = device_adam(saved["names"])
            optimizer.load_state_dict(saved)
            seen = (saved["step"], saved["skipped"], 0.0)
        elif not on_device and saved is not None:
            from .optim import load_into_torch_adam
            if state["optimizer_kind"] == "torch":
                optimizer.load_state_dict(state["optimizer"])
            else:
                load_into_torch_adam(optimizer, saved, [named[n] for n in saved["names"]])
        averages = list(state["averages"])
        set_generator_states(rng, state["generators"], device)
        start_epoch = state["epoch"]
    model.train()
    for epoch in range(start_epoch, epochs):
        if not on_device:
            for group in optimizer.param_groups:
                group["lr"] = learning_rate(lr, epoch)
        elif optimizer is not None:
            optimizer.lr = learning_rate(lr, epoch)
        losses, terms = [], []
        for plan in clips.epoch(batch_size, rng, crop):
            if optimizer is not None:
                optimizer.zero_grad()
            x, mvs0, mvs1, pms, rms, ufs, hr = clips.batch(plan, crop)
            sr, _ = model(x, mvs0, mvs1, pms, rms, ufs)
            loss = charbonnier(sr, hr)
            if lpips is not None or ffl_weight or ssim_weight:
                parts = [loss.detach()]
                if lpips is not None:
                    perc = lpips_loss(sr, hr, lpips).sum()
                    loss = loss + lpips_weight * perc
                    parts.append(perc.detach())
                if ffl_weight:
                    freq = focal_frequency_loss(sr, hr, ffl_alpha).sum()
                    loss = loss + ffl_weight * freq
                    parts.append(freq.detach())
                if ssim_weight:
                    struct = (ssim_loss if ssim_scales == 1 else msssim_loss)(sr, hr).sum()
                    loss = loss + ssim_weight * struct
                    parts.append(struct.detach())
                terms.append(torch.stack(parts))
            losses.append(loss.detach())
            loss.backward()
            if optimizer is None:
                optimizer = device_adam([n for n, p in named.items() if p.grad is not None])
                optimizer.lr = learning_rate(lr, epoch)
            optimizer.step()
        if on_device:                                                         # the same read, the optimizer's counters and norms behind the losses
            per_batch = torch.cat([torch.stack(losses).double(), optimizer.counters.double(), optimizer.norm_sum.reshape(1)]).cpu().tolist()
            now = (int(per_batch[-3]), int(per_batch[-2]), per_batch[-1])
            del per_batch[-3:]
        else:
            per_batch = torch.stack(losses).cpu().tolist()                    # the epoch's one read of the device
        averages.append(round(sum(per_batch) / len(per_batch), 5))
        line = '[%s] Epoch: %d/%d | average epoch loss: %f' % (datetime.now().strftime("%d/%m/%Y %H:%M:%S"), epoch + 1, epochs, averages[-1])
        if terms:
            names = ['charbonnier'] + ['lpips'] * (lpips is not None) + ['ffl'] * bool(ffl_weight) + ['ssim' if ssim_scales == 1 else 'msssim'] * bool(ssim_weight)
            line += ''.join(' | %s: %f' % nv for nv in zip(names, torch.stack(terms).mean(dim=0).cpu().tolist()))
        if on_device:
            made = now[0] - seen[0]
            line += ' | grad norm: %f' % ((now[2] - seen[2]) / made if made else float("nan"))
            if now[1] != seen[1]:
                line += ' | skipped: %d' % (now[1] - seen[1])
            seen = now
        log(line)
        if (epoch + 1) % val_itv == 0:
            torch.save(model.state_dict(), os.path.join(out_dir, "ckpt", "epoch-%d.pth" % (epoch + 1)))
            log('Saved model. lr %f' % learning_rate(lr, epoch))
            if val is not None:
                model.eval()
                with torch.no_grad():
                    r = evaluate_sequence(model, val[0], val[1], gt_dir=val[2], coding=val_coding)
                model.train()
                log('PSNR:%f, SSIM: %f' % (r.mean_psnr, r.mean_ssim))
            if save_state:                # after the validation: whatever that drew from a generator is part of the state
                write_state(state_path(out_dir, epoch + 1), optimizer, kind, epoch + 1, averages, rng, device, run)
    return averages
