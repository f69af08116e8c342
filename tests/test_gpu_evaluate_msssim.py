"""evaluate_sequence / evaluate_yuv with ``msssim=True`` on the GPU: T = 3 frames of 48x52 (a 192x208 result, 184x200 inside the
border, the smallest the five scales allow at these LR sizes), chunk 2, so the last chunk is ragged.  The synthetic writers' ground
truth is independent noise, for which MS-SSIM is ill-conditioned; each case makes its own: the frames a first run writes, plus noise."""
import filecmp
import os

import numpy as np
import pytest
import torch

import msssim_ref as ref

pytestmark = pytest.mark.gpu
T, H, W, CHUNK = 3, 48, 52, 2
SEED = 4321
SSIM_TOL = 1e-9       # per mean, as tests/test_gpu_msssim.py; the combined value is held to its first-order propagation


@pytest.fixture(scope="module")
def model_and_noise():
    from arch.SIDECVSR_our import CVSR_V8
    from oracle.cvsr_v8_ref import make_inputs, make_state_dict
    m = CVSR_V8()
    m.load_state_dict(make_state_dict(21, perturb=True), strict=True)
    noise = [make_inputs(1, 48, 56, 900 + t)["gumbel_u"] for t in range(T)]        # the frames are padded to 48x56 inside
    return m.cuda().eval(), [[u.cuda() for u in six] for six in noise]


def _noisy(frames: np.ndarray, peak: int, sigma: float) -> np.ndarray:
    rs = np.random.RandomState(7)
    return np.clip(frames.astype(np.int64) + np.rint(sigma * rs.randn(*frames.shape)).astype(np.int64), 0, peak).astype(frames.dtype)


def _check(r_on, r_off, names, frames, gt, peak, log):
    """The MS-SSIM figures of the run with the option against the oracle on the written frames; everything else against the run
    without it."""
    assert r_on.msssim.dtype == np.float64 and r_on.msssim.shape == (T,)
    assert len(r_off.msssim) == 0 and np.isnan(r_off.mean_msssim)
    for t in range(T):
        want = ref.components(frames[t], gt[t], 4, peak)
        assert want.min() >= 0.1, want
        bound = ref.propagated_bound(want, SSIM_TOL)
        print(f"frame {t}: MS-SSIM {r_on.msssim[t]!r}, oracle {ref.combine(want)!r}, smallest component {want.min():.4f}, bound {bound:.2e}")
        assert abs(r_on.msssim[t] - ref.combine(want)) < bound
    assert r_on.mean_msssim == r_on.msssim.sum() / T
    assert log(r_on, "s") == log(r_off, "s") + " MS-SSIM: %.5f" % r_on.mean_msssim
    for name in names:
        x, y = getattr(r_on, name), getattr(r_off, name)
        assert x.shape == y.shape and np.all(x == y), name
    assert len(getattr(r_on, names[0])) == T


def test_png_directories(model_and_noise, tmp_path):
    from cdfo_amd.evaluate import evaluate_sequence, format_log, write_synthetic_sequence
    from cdfo_amd.priors import read_gray_png, write_gray_png
    model, noise = model_and_noise
    lr_dir, side, _ = write_synthetic_sequence(str(tmp_path / "seq"), T, H, W, seed=11, gt=False)

    def run(save, **kw):
        torch.manual_seed(SEED)
        return evaluate_sequence(model, lr_dir, side, save_dir=str(tmp_path / save), chunk=CHUNK, gumbel_uniform=noise, **kw)

    first = run("first", msssim=True)                                         # no ground truth: nothing to report
    assert len(first.msssim) == 0 and np.isnan(first.mean_msssim) and "MS-SSIM" not in format_log(first, "s")
    frames = np.stack([read_gray_png(str(tmp_path / "first" / ("%05d.png" % t))) for t in range(T)])
    assert frames.shape == (T, 4 * H, 4 * W)
    gt, gt_dir = _noisy(frames, 255, 20), str(tmp_path / "gt")
    os.makedirs(gt_dir)
    for t in range(T):
        write_gray_png(os.path.join(gt_dir, "%05d.png" % t), gt[t])
    r_off, r_on = run("off", gt_dir=gt_dir), run("on", gt_dir=gt_dir, msssim=True)
    _check(r_on, r_off, ("psnr", "ssim"), frames, gt, 255, format_log)
    for t in range(T):
        assert filecmp.cmp(str(tmp_path / "on" / ("%05d.png" % t)), str(tmp_path / "off" / ("%05d.png" % t)), shallow=False)
        assert filecmp.cmp(str(tmp_path / "on" / ("%05d.png" % t)), str(tmp_path / "first" / ("%05d.png" % t)), shallow=False)


@pytest.mark.parametrize("pix_fmt,peak,sigma", [("yuv420p", 255, 20), ("yuv420p10le", 1023, 80)])
def test_raw_yuv(model_and_noise, tmp_path, pix_fmt, peak, sigma):
    from cdfo_amd.evaluate import evaluate_yuv, format_log_yuv, write_synthetic_sequence_yuv
    from cdfo_amd.yuv import YuvReader, YuvWriter
    model, noise = model_and_noise
    lr_yuv, side, _ = write_synthetic_sequence_yuv(str(tmp_path / "seq"), T, H, W, seed=11, gt=False, pix_fmt=pix_fmt)

    def run(save, **kw):
        torch.manual_seed(SEED)
        return evaluate_yuv(model, lr_yuv, W, H, side, save_yuv=str(tmp_path / save), chunk=CHUNK, gumbel_uniform=noise, pix_fmt=pix_fmt,
                            **kw)

    first = run("first.yuv", msssim=True)
    assert len(first.msssim) == 0 and np.isnan(first.mean_msssim) and "MS-SSIM" not in format_log_yuv(first, "s")
    with YuvReader(str(tmp_path / "first.yuv"), 4 * W, 4 * H, pix_fmt) as f:
        assert f.frames == T
        frames = np.array(f.y(0, T))
    gt, gt_yuv = _noisy(frames, peak, sigma), str(tmp_path / "gt.yuv")
    rc = np.random.RandomState(8)
    with YuvWriter(gt_yuv, 4 * W, 4 * H, pix_fmt) as w:
        for t in range(T):
            w.append(gt[t], *(rc.randint(0, peak + 1, (2 * H, 2 * W)).astype(gt.dtype) for _ in range(2)))
    r_off, r_on = run("off.yuv", gt_yuv=gt_yuv), run("on.yuv", gt_yuv=gt_yuv, msssim=True)
    _check(r_on, r_off, ("psnr_y", "psnr_u", "psnr_v", "ssim_y", "psnr_yuv"), frames, gt, peak, format_log_yuv)
    assert filecmp.cmp(str(tmp_path / "on.yuv"), str(tmp_path / "off.yuv"), shallow=False)
    assert filecmp.cmp(str(tmp_path / "on.yuv"), str(tmp_path / "first.yuv"), shallow=False)
