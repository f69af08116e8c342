"""`train.fit` with the structural term: two epochs at one scale on the clip set of tests/test_gpu_ffl_loss.py, one step of five scales
at ``crop=48``, the log line, two runs from one seed, a run without the keyword, and a state
file that resumes and refuses another ``ssim_weight``.

`fit` takes five scales from ``crop=44`` (HR 176 x 176, tests/test_ssim_loss_cpu.py), but ``CVSR_V8``'s window attention takes LR crops
whose sides are multiples of 8 only, so the smallest crop a step can run at is 48 (HR 192 x 192)."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_FITS = {}


def _model(seed=1):
    from arch.SIDECVSR_our import CVSR_V8
    torch.manual_seed(seed)
    return CVSR_V8(SCGs=8).cuda()


def _clips():
    from cdfo_amd.train_data import ClipSet, synthetic_arrays
    return ClipSet.from_arrays(*synthetic_arrays(2, 8, 20, 20, seed=1))


def _fit(tag, tmp_path_factory, **kw):
    """(averages, log lines, state dict on the host) of `train.fit` for two epochs of one batch of two 16 x 16 crops (HR 64 x 64) on a
    synthetic set, from the seed 1; run once per tag and shared.  The sizes are those of tests/test_gpu_ffl_loss.py."""
    if tag not in _FITS:
        from cdfo_amd.train import fit
        model, lines = _model(), []
        averages = fit(model, _clips(), 2, str(tmp_path_factory.mktemp(tag)), batch_size=2, crop=16, val_itv=10, log=lines.append, **kw)
        _FITS[tag] = averages, lines, {k: v.detach().cpu() for k, v in model.state_dict().items()}
    return _FITS[tag]


def test_fit_with_and_without_the_term(tmp_path_factory):
    a1, l1, s1 = _fit("ssim-a", tmp_path_factory, ssim_weight=0.5)
    a0, l0, s0 = _fit("plain", tmp_path_factory)
    az, lz, sz = _fit("zero", tmp_path_factory, ssim_weight=0.0, ssim_scales=1)
    assert len(a1) == 2 and np.isfinite(a1).all() and len(l1) == 2 and len(l0) == 2
    assert all(bool(torch.isfinite(v).all()) for v in s1.values()) and any(not torch.equal(s1[k], s0[k]) for k in s1)
    for ln, avg in zip(l1, a1):
        m = re.search(r"average epoch loss: ([0-9.]+) \| charbonnier: ([0-9.]+) \| ssim: ([0-9.]+)$", ln)
        assert m and abs(float(m.group(1)) - avg) < 1e-5
        assert 0 < float(m.group(3)) <= 2 * 2 and abs(float(m.group(2)) + 0.5 * float(m.group(3)) - avg) < 1e-3 * avg
    # the plain run: no suffix, and lines and averages are what the keyword's zero gives (the first epoch in every digit; the second
    # follows a step whose flow-warp adjoint adds with fp32 atomics in a plain run, as tests/test_gpu_ffl_loss.py explains)
    assert all(re.search(r"average epoch loss: [0-9.]+$", ln) for ln in l0 + lz)
    strip = lambda lines: [ln.split("] ", 1)[1] for ln in lines]                               # noqa: E731  (the date in front)
    assert strip(l0)[0] == strip(lz)[0] and a0[0] == az[0] and abs(a0[1] - az[1]) <= 1e-5 * a0[1]
    assert strip(l0)[1].split(": ")[:2] == strip(lz)[1].split(": ")[:2]


def test_fit_beside_the_frequency_term(tmp_path_factory):
    avgs, lines, sd = _fit("ffl-ssim", tmp_path_factory, ffl_weight=2.0, ssim_weight=0.5)
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
    for ln, avg in zip(lines, avgs):
        m = re.search(r"average epoch loss: ([0-9.]+) \| charbonnier: ([0-9.]+) \| ffl: ([0-9.]+) \| ssim: ([0-9.]+)$", ln)
        assert m and abs(float(m.group(1)) - avg) < 1e-5 and float(m.group(3)) > 0 and float(m.group(4)) > 0
        assert abs(float(m.group(2)) + 2.0 * float(m.group(3)) + 0.5 * float(m.group(4)) - avg) < 1e-3 * avg


def test_fit_twice_from_one_seed_gives_equal_weights(tmp_path_factory):
    _, _, s1 = _fit("ssim-a", tmp_path_factory, ssim_weight=0.5)
    _, _, s2 = _fit("ssim-b", tmp_path_factory, ssim_weight=0.5)
    differ = [k for k in s1 if not torch.equal(s1[k], s2[k])]
    print(f"{len(differ)} of {len(s1)} tensors differ between two runs from one seed")
    assert not differ


def test_one_step_of_five_scales(tmp_path):
    """crop = 48: the smallest multiple of 8 (the model's 8 x 8 attention windows) from 44 up."""
    from cdfo_amd.train import fit
    from cdfo_amd.train_data import ClipSet, synthetic_arrays
    clips = ClipSet.from_arrays(*synthetic_arrays(1, 8, 52, 52, seed=1))
    model, lines = _model(), []
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    averages = fit(model, clips, 1, str(tmp_path), batch_size=1, crop=48, val_itv=10, log=lines.append, ssim_weight=0.5, ssim_scales=5)
    assert len(averages) == 1 and len(lines) == 1
    m = re.search(r"average epoch loss: ([0-9.]+) \| charbonnier: ([0-9.]+) \| msssim: ([0-9.]+)$", lines[0])
    assert m and 0 < float(m.group(3)) <= 1 and abs(float(m.group(2)) + 0.5 * float(m.group(3)) - averages[0]) < 1e-3 * averages[0]
    after = model.state_dict()
    assert all(bool(torch.isfinite(v).all()) for v in after.values()) and any(not torch.equal(after[k], before[k]) for k in after)


def test_a_saved_state_resumes_and_refuses_another_weight(tmp_path):
    from cdfo_amd.train import fit
    clips = _clips()
    kw = dict(batch_size=2, crop=16, val_itv=1, save_state=True, ssim_weight=0.5, log=lambda s: None)
    straight, halves = str(tmp_path / "straight"), str(tmp_path / "halves")
    want = fit(_model(), clips, 2, straight, **kw)
    first = fit(_model(), clips, 1, halves, **kw)
    state = os.path.join(halves, "ckpt", "epoch-1.state.pth")
    run = torch.load(state)["run"]
    assert first == want[:1] and run["ssim_weight"] == 0.5 and "ssim_scales" not in run              # a default is not written
    for change, name in ((dict(ssim_weight=0.25), "ssim_weight"), (dict(ssim_weight=0.0), "ssim_weight")):
        with pytest.raises(ValueError, match=rf"\b{name} = 0.5, this call has {name} = "):
            fit(_model(), clips, 2, str(tmp_path / "other"), resume=state, **dict(kw, **change))
    assert not os.path.exists(tmp_path / "other")
    got = fit(_model(seed=77), clips, 2, halves, resume=state, **kw)                               # a fresh model: other weights
    assert got == want
    a = torch.load(os.path.join(straight, "ckpt", "epoch-2.pth"), map_location="cpu")
    b = torch.load(os.path.join(halves, "ckpt", "epoch-2.pth"), map_location="cpu")
    assert all(torch.equal(a[k], b[k]) for k in a)
