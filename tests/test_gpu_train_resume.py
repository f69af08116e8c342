"""`cdfo_amd.train.fit` stopped and continued: four epochs straight against two epochs plus ``resume``, with either optimizer, bit for
bit; the state file; the default call, which writes none and logs what it always did; the errors of ``resume``; the device optimizer's
log line."""
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
KW = dict(batch_size=2, crop=8, val_itv=1)


def _clips():
    from cdfo_amd.train_data import ClipSet, synthetic_arrays
    return ClipSet.from_arrays(*synthetic_arrays(4, 8, 16, 16, seed=1))


def _model(seed=1):
    from arch.SIDECVSR_our import CVSR_V8
    torch.manual_seed(seed)
    return CVSR_V8(SCGs=8).cuda()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu().reshape(-1).view(torch.uint8), b.cpu().reshape(-1).view(torch.uint8))


def _tensors(x):
    if isinstance(x, torch.Tensor):
        return [x]
    if isinstance(x, dict):
        return [t for k in x for t in _tensors(x[k])]
    if isinstance(x, (list, tuple)):
        return [t for v in x for t in _tensors(v)]
    return []


@pytest.mark.parametrize("optimizer", ["device", "torch"])
def test_two_epochs_and_a_resume_equal_four_epochs(tmp_path, optimizer):
    from cdfo_amd.train import fit
    clips = _clips()
    straight, halves = str(tmp_path / "straight"), str(tmp_path / "halves")
    kw = dict(KW, deterministic=True, save_state=True, optimizer=optimizer, log=lambda s: None)
    want = fit(_model(), clips, 4, straight, **kw)
    first = fit(_model(), clips, 2, halves, **kw)
    assert first == want[:2]
    got = fit(_model(seed=77), clips, 4, halves, resume=os.path.join(halves, "ckpt", "epoch-2.state.pth"), **kw)   # a fresh model: other weights
    assert got == want and len(got) == 4                                                  # the averages of epochs 3 and 4 among them
    for n in (3, 4):
        a = torch.load(os.path.join(straight, "ckpt", f"epoch-{n}.pth"), map_location="cpu")
        b = torch.load(os.path.join(halves, "ckpt", f"epoch-{n}.pth"), map_location="cpu")
        assert len(a) == len(b) == 261 and all(_same_bits(a[k], b[k]) for k in a)
        sa = torch.load(os.path.join(straight, "ckpt", f"epoch-{n}.state.pth"))           # torch.load's defaults read a state file
        sb = torch.load(os.path.join(halves, "ckpt", f"epoch-{n}.state.pth"))
        assert sa["optimizer_kind"] == sb["optimizer_kind"] == optimizer and sa["epoch"] == sb["epoch"] == n
        ta, tb = _tensors(sa["optimizer"]), _tensors(sb["optimizer"])
        assert len(ta) == len(tb) >= 2 * 257 and all(_same_bits(x, y) for x, y in zip(ta, tb))
        assert sa["averages"] == sb["averages"] == want[:n] and sa["run"] == sb["run"]
        assert sa["generators"]["numpy"] == sb["generators"]["numpy"]
        assert all(_same_bits(sa["generators"][k], sb["generators"][k]) for k in ("torch_cpu", "torch_device"))
    if optimizer == "device":
        assert sa["optimizer"]["step"] == 4 * 2 and sa["optimizer"]["skipped"] == 0       # two batches an epoch
    assert set(sa["run"]) == {"batch_size", "crop", "lr", "weight_decay", "seed", "coding", "lpips_weight", "ffl_weight", "ffl_alpha",
                              "max_grad_norm"}


def test_the_default_call_writes_no_state_file_and_logs_the_old_line(tmp_path):
    from cdfo_amd.train import fit
    lines = []
    averages = fit(_model(), _clips(), 2, str(tmp_path), log=lines.append, **KW)
    assert sorted(os.listdir(tmp_path / "ckpt")) == ["epoch-1.pth", "epoch-2.pth"]
    epoch_lines = [ln for ln in lines if "average epoch loss" in ln]
    assert len(epoch_lines) == 2 and len(averages) == 2
    for e, ln in enumerate(epoch_lines):
        assert re.fullmatch(r"\[\d\d/\d\d/\d{4} \d\d:\d\d:\d\d\] Epoch: %d/2 \| average epoch loss: [0-9.]+" % (e + 1), ln), ln
    assert [ln for ln in lines if ln.startswith("Saved model.")] == ["Saved model. lr 0.000100"] * 2
    assert len(lines) == 4


def test_resume_refuses_another_run_and_a_lone_state_file(tmp_path):
    from cdfo_amd.train import fit
    clips = _clips()
    out = str(tmp_path / "run")
    fit(_model(), clips, 1, out, save_state=True, optimizer="device", max_grad_norm=5.0, log=lambda s: None, **KW)
    state = os.path.join(out, "ckpt", "epoch-1.state.pth")
    base = dict(KW, optimizer="device", max_grad_norm=5.0, resume=state, log=lambda s: None)
    model = _model()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    for change, name in ((dict(batch_size=4), "batch_size"), (dict(crop=4), "crop"), (dict(lr=1e-3), "lr"), (dict(weight_decay=0.0), "weight_decay"),
                         (dict(seed=5), "seed"), (dict(max_grad_norm=None), "max_grad_norm"), (dict(ffl_weight=1.0), "ffl_weight"),
                         (dict(batch_size=4, seed=5), "batch_size")):
        with pytest.raises(ValueError, match=rf"\b{name} = "):
            fit(model, clips, 3, str(tmp_path / "other"), **dict(base, **change))
    with pytest.raises(ValueError, match="nothing to run"):
        fit(model, clips, 1, str(tmp_path / "other"), **base)
    with pytest.raises(ValueError, match="start_epoch"):
        fit(model, clips, 3, str(tmp_path / "other"), start_epoch=1, **base)
    os.rename(os.path.join(out, "ckpt", "epoch-1.pth"), os.path.join(out, "ckpt", "elsewhere.pth"))
    with pytest.raises(ValueError, match="weights .* missing"):
        fit(model, clips, 3, str(tmp_path / "other"), **base)
    assert not os.path.exists(tmp_path / "other")                                         # all of it before the first batch
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())


def test_the_device_optimizer_logs_its_gradient_norm(tmp_path):
    from cdfo_amd.train import fit
    model = _model()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    lines = []
    fit(model, _clips(), 2, str(tmp_path), optimizer="device", log=lines.append, **KW)
    epoch_lines = [ln for ln in lines if "average epoch loss" in ln]
    assert len(epoch_lines) == 2
    for ln in epoch_lines:
        m = re.search(r"average epoch loss: [0-9.]+ \| grad norm: ([0-9.]+)$", ln)
        assert m and float(m.group(1)) > 0 and "skipped" not in ln, ln
    assert sorted(os.listdir(tmp_path / "ckpt")) == ["epoch-1.pth", "epoch-2.pth"]
    after = model.state_dict()
    assert any(not torch.equal(after[k], before[k]) for k in after)                      # the weights moved
