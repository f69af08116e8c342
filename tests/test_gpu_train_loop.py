"""The training loop (cdfo_amd/train.py::fit; train_LD_37.py:359-402) on a synthetic clip set: device batches, the device loss, the
HIP forward and backward, Adam, the per-epoch log line and the checkpoint."""
import re

import numpy as np
import pytest
import torch


def test_learning_rate_rule():
    """MultiStepLR([2000], 0.5) stepped at the top of each epoch: 0-based epoch 1998 still runs at lr0, epoch 1999 at half of it."""
    from cdfo_amd.train import learning_rate
    assert learning_rate(1e-4, 0) == 1e-4 and learning_rate(1e-4, 1998) == 1e-4
    assert learning_rate(1e-4, 1999) == 0.5e-4 and learning_rate(1e-4, 29999) == 0.5e-4


@pytest.mark.gpu
def test_fit_trains_logs_and_checkpoints(tmp_path):
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd.train import fit
    from cdfo_amd.train_data import ClipSet, synthetic_arrays
    torch.manual_seed(1)
    clips = ClipSet.from_arrays(*synthetic_arrays(4, 8, 16, 16, seed=1))
    model = CVSR_V8(SCGs=8).cuda()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    from cdfo_amd.evaluate import write_synthetic_sequence
    val = write_synthetic_sequence(str(tmp_path / "val"), 3, 16, 20, seed=2)
    lines = []
    averages = fit(model, clips, 2, str(tmp_path), batch_size=2, crop=8, val_itv=1, val=val, log=lines.append)
    metrics = [re.fullmatch(r"PSNR:([0-9.]+), SSIM: ([0-9.]+)", ln) for ln in lines if ln.startswith("PSNR:")]
    assert len(metrics) == 2 and all(m and np.isfinite(float(m.group(1))) for m in metrics)      # one validation per checkpoint
    assert len(averages) == 2 and np.isfinite(averages).all() and all(a > 0 for a in averages)
    epoch_lines = [ln for ln in lines if "average epoch loss" in ln]
    assert len(epoch_lines) == 2
    for e, ln in enumerate(epoch_lines):
        m = re.search(r"Epoch: (\d+)/(\d+) \| average epoch loss: ([0-9.]+)$", ln)
        assert m and (int(m.group(1)), int(m.group(2))) == (e + 1, 2) and abs(float(m.group(3)) - averages[e]) < 1e-5
    assert model.training
    for n in (1, 2):
        sd = torch.load(str(tmp_path / "ckpt" / f"epoch-{n}.pth"), map_location="cpu")
        assert len(sd) == 261
        CVSR_V8(SCGs=8).load_state_dict(sd, strict=True)
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
    assert any(not torch.equal(sd[k], before[k].cpu()) for k in sd)          # the optimiser moved the weights
