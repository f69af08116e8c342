"""NIQE end to end on the GPU: `metrics.niqe_u8` on the fixture frames against the numpy statement (tests/niqe_ref.py) and the
reference's recorded scores, and ``niqe=`` in both evaluators.

The score bound against the statement is derived on the CPU, not from the device: every feature of the statement is moved by 1e-9
relative (the kernels' bound, tests/test_gpu_niqe_kernels.py) with a random sign, 100 seeded draws per frame, and 10 x the largest
change of the score is the bound (`niqe_ref.perturbation_bound`).  On the committed fixture that is, per frame a .. f:
1.0e-06, 9.8e-07, 7.7e-07, 3.1e-06, 1.5e-06, 1.2e-06 on scores of 13.5 .. 26.9.  Against the reference's scores the bound is the CPU
test's (3.24e-06, the fp32 resize floor) plus that one, with the model rounded to fp32 the way the reference holds it.

Evaluators: T = 9 frames of 48 x 56 (a 192 x 224 result, region 192 x 192, 2 x 2 blocks), chunks of 4, so the last chunk is ragged
and holds one frame."""
import os

import numpy as np
import pytest
import torch

import niqe_ref as ref
from test_niqe_cpu import SCORE_ABS

pytestmark = pytest.mark.gpu
T, H, W, CHUNK = 9, 48, 56, 4
SEED = 4321


@pytest.mark.parametrize("group", ["bcf", "a", "d", "e"])
def test_scores_match_the_statement_and_the_reference(group):
    from cdfo_amd import metrics as M
    z = ref.golden()
    if len(group) == 1:
        frames = torch.from_numpy(z["frame_" + group]).cuda()
    else:                                                                  # c is smaller than b and f: pad it with other content
        buf = np.random.RandomState(3).randint(0, 256, (3, 200, 300)).astype(np.uint8)
        for k, n in enumerate(group):
            f = z["frame_" + n]
            buf[k, :f.shape[0], :f.shape[1]] = f
        frames = torch.from_numpy(buf).cuda()
    got = M.niqe_u8(frames, M.niqe_params(ref.model()))
    like_ref = M.niqe_u8(frames, ref.model(as_reference=True))
    assert got.dtype == np.float64 and got.shape == (len(group),)
    for k, n in enumerate(group):
        want, bound = ref.score(ref.golden_pieces(n)["features"], *ref.model()), ref.perturbation_bound(n)
        print(f"{n}: device {got[k]!r}, statement {want!r}, |difference| {abs(got[k] - want):.2e}, bound {bound:.2e}; against the "
              f"reference's {float(z['score_' + n])!r}: {abs(like_ref[k] - z['score_' + n]):.2e}, bound {SCORE_ABS + bound:.2e}")
        assert 1e-8 < bound < 1e-4
        assert abs(got[k] - want) <= bound
        assert abs(like_ref[k] - z["score_" + n]) <= SCORE_ABS + bound


@pytest.fixture(scope="module")
def model_and_noise():
    from arch.SIDECVSR_our import CVSR_V8
    from oracle.cvsr_v8_ref import make_inputs, make_state_dict
    m = CVSR_V8()
    m.load_state_dict(make_state_dict(21, perturb=True), strict=True)
    noise = [make_inputs(1, H, W, 900 + t)["gumbel_u"] for t in range(T)]
    return m.cuda().eval(), [[u.cuda() for u in six] for six in noise]


def _check(r_gt, r_gt_off, r_free, frames, params, names, log):
    from cdfo_amd import metrics as M
    for r in (r_gt, r_free):
        assert r.niqe.dtype == np.float64 and r.niqe.shape == (T,) and np.isfinite(r.niqe).all()
        assert r.mean_niqe == r.niqe.sum() / T
    assert np.array_equal(r_gt.niqe.view(np.uint64), r_free.niqe.view(np.uint64))          # ground truth or not: the same bits
    assert np.array_equal(r_gt.niqe.view(np.uint64), M.niqe_u8(torch.from_numpy(frames).cuda(), params).view(np.uint64))
    assert len(r_gt_off.niqe) == 0 and np.isnan(r_gt_off.mean_niqe)
    for name in names:                                                     # PSNR and SSIM are unchanged by the option, bit for bit
        x, y = getattr(r_gt, name), getattr(r_gt_off, name)
        assert len(x) == T and x.shape == y.shape and np.all(x == y), name
        assert len(getattr(r_free, name)) == 0
    assert "NIQE" not in log(r_gt_off, "s") and log(r_gt, "s") == log(r_gt_off, "s") + " NIQE: %.5f" % r_gt.mean_niqe
    assert log(r_free, "s").endswith(" NIQE: %.5f" % r_free.mean_niqe)


def test_png_directories(model_and_noise, tmp_path):
    from cdfo_amd import metrics as M
    from cdfo_amd.evaluate import evaluate_sequence, format_log, write_synthetic_sequence
    from cdfo_amd.priors import read_gray_png
    model, noise = model_and_noise
    lr_dir, side, gt_dir = write_synthetic_sequence(str(tmp_path / "seq"), T, H, W, seed=11)
    np.savez(tmp_path / "model.npz", mu_prisparam=ref.model()[0], cov_prisparam=ref.model()[1])
    params = M.niqe_params(str(tmp_path / "model.npz"))

    def run(**kw):
        torch.manual_seed(SEED)
        return evaluate_sequence(model, lr_dir, side, chunk=CHUNK, gumbel_uniform=noise, **kw)

    r_free = run(save_dir=str(tmp_path / "out"), niqe=str(tmp_path / "model.npz"))            # a path; no ground truth
    r_gt, r_gt_off = run(gt_dir=gt_dir, niqe=params), run(gt_dir=gt_dir)                       # a loaded model
    frames = np.stack([read_gray_png(str(tmp_path / "out" / ("%05d.png" % t))) for t in range(T)])
    assert frames.shape == (T, 4 * H, 4 * W)
    print("NIQE per frame:", " ".join("%.4f" % v for v in r_free.niqe))
    _check(r_gt, r_gt_off, r_free, frames, params, ("psnr", "ssim"), format_log)


def test_raw_yuv(model_and_noise, tmp_path):
    from cdfo_amd import metrics as M
    from cdfo_amd.evaluate import evaluate_yuv, format_log_yuv, write_synthetic_sequence_yuv
    from cdfo_amd.yuv import YuvReader
    model, noise = model_and_noise
    lr_yuv, side, gt_yuv = write_synthetic_sequence_yuv(str(tmp_path / "seq"), T, H, W, seed=11)
    params = M.niqe_params(ref.model())

    def run(**kw):
        torch.manual_seed(SEED)
        return evaluate_yuv(model, lr_yuv, W, H, side, chunk=CHUNK, gumbel_uniform=noise, **kw)

    r_free = run(save_yuv=str(tmp_path / "out.yuv"), niqe=ref.model())                         # a pair of arrays
    r_gt, r_gt_off = run(gt_yuv=gt_yuv, niqe=params), run(gt_yuv=gt_yuv)
    with YuvReader(str(tmp_path / "out.yuv"), 4 * W, 4 * H, "yuv420p") as f:
        assert f.frames == T
        frames = np.array(f.y(0, T))
    _check(r_gt, r_gt_off, r_free, frames, params, ("psnr_y", "psnr_u", "psnr_v", "ssim_y", "psnr_yuv"), format_log_yuv)


def test_refusals_before_any_launch(model_and_noise, tmp_path):
    from cdfo_amd.evaluate import (evaluate_sequence, evaluate_yuv, write_synthetic_sequence, write_synthetic_sequence_yuv)
    model, _ = model_and_noise
    lr_yuv, side, _ = write_synthetic_sequence_yuv(str(tmp_path / "ten"), 2, H, W, seed=3, gt=False, pix_fmt="yuv420p10le")
    with pytest.raises(ValueError, match="8-bit"):
        evaluate_yuv(model, lr_yuv, W, H, side, pix_fmt="yuv420p10le", niqe=ref.model())
    lr_dir, side, _ = write_synthetic_sequence(str(tmp_path / "small"), 2, 20, 30, seed=3, gt=False)      # an 80 x 120 result
    with pytest.raises(ValueError, match="96 x 96"):
        evaluate_sequence(model, lr_dir, side, niqe=ref.model())
    lr_yuv, side, _ = write_synthetic_sequence_yuv(str(tmp_path / "small_yuv"), 2, 20, 30, seed=3, gt=False)
    with pytest.raises(ValueError, match="96 x 96"):
        evaluate_yuv(model, lr_yuv, 30, 20, side, niqe=ref.model())
    with pytest.raises(ValueError):
        evaluate_sequence(model, lr_dir, side, niqe=(np.zeros(35), np.zeros((36, 36))))
