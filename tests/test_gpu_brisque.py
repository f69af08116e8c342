"""BRISQUE end to end on the GPU: `metrics.brisque_u8` on the fixture frames against the numpy statement (tests/brisque_ref.py) and the
reference's recorded scores, and ``brisque=`` in both evaluators.

The score bound against the statement is derived on the CPU, not from the device: every feature of the statement is moved by 1e-9
relative (the kernels' bound, tests/test_gpu_brisque_kernels.py) with a random sign, 100 seeded draws per frame, and 10 x the largest
change of the score is the bound (`brisque_ref.perturbation_bound`).  On the committed fixture that is, per frame a .. e:
2.7e-06, 3.2e-06, 2.4e-06, 2.9e-06, 2.2e-06 on scores of 53 .. 96 (the support vectors' coefficients sum to 7.4e5 in magnitude).
Against the reference's scores the bound is the CPU test's (3.52e-03, the reference's fp32 kernel sum) plus that one, with the
ranges, gamma and rho rounded to fp32 the way the reference holds them.

Evaluators: T = 9 frames of 48 x 56 (a 192 x 224 result), chunks of 4, so the last chunk is ragged and holds one frame."""
import numpy as np
import pytest
import torch

import brisque_ref as ref
import niqe_ref
from test_brisque_cpu import SCORE_ABS

pytestmark = pytest.mark.gpu
T, H, W, CHUNK = 9, 48, 56, 4
SEED = 4321


@pytest.mark.parametrize("group", ["cdz", "a", "b", "e"])
def test_scores_match_the_statement_and_the_reference(group):
    from cdfo_amd import metrics as M
    z = ref.golden()
    frames = torch.from_numpy(np.stack([z["frame_" + n] for n in group])).cuda()
    got = M.brisque_u8(frames, M.brisque_params(ref.model()))
    like_ref = M.brisque_u8(frames, ref.model(as_reference=True))
    assert got.dtype == np.float64 and got.shape == (len(group),)
    for k, n in enumerate(group):
        if n == "z":
            assert np.isnan(got[k]) and np.isnan(like_ref[k])
            continue
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
        assert r.brisque.dtype == np.float64 and r.brisque.shape == (T,) and np.isfinite(r.brisque).all()
        assert r.mean_brisque == r.brisque.sum() / T
        assert len(r.niqe) == 0 and np.isnan(r.mean_niqe)
    assert np.array_equal(r_gt.brisque.view(np.uint64), r_free.brisque.view(np.uint64))    # ground truth or not: the same bits
    assert np.array_equal(r_gt.brisque.view(np.uint64), M.brisque_u8(torch.from_numpy(frames).cuda(), params).view(np.uint64))
    assert len(r_gt_off.brisque) == 0 and np.isnan(r_gt_off.mean_brisque)
    for name in names:                                                     # PSNR and SSIM are unchanged by the option, bit for bit
        x, y = getattr(r_gt, name), getattr(r_gt_off, name)
        assert len(x) == T and x.shape == y.shape and np.all(x == y), name
        assert len(getattr(r_free, name)) == 0
    assert "BRISQUE" not in log(r_gt_off, "s") and log(r_gt, "s") == log(r_gt_off, "s") + " BRISQUE: %.5f" % r_gt.mean_brisque
    assert log(r_free, "s").endswith(" BRISQUE: %.5f" % r_free.mean_brisque)


def _save_model(path):
    sv, coef, ranges, gamma, rho = ref.model()
    np.savez(path, sv=sv, sv_coef=coef, feature_ranges=ranges, gamma=gamma, rho=rho)
    return str(path)


def test_png_directories(model_and_noise, tmp_path):
    from cdfo_amd import metrics as M
    from cdfo_amd.evaluate import evaluate_sequence, format_log, write_synthetic_sequence
    from cdfo_amd.priors import read_gray_png
    model, noise = model_and_noise
    lr_dir, side, gt_dir = write_synthetic_sequence(str(tmp_path / "seq"), T, H, W, seed=11)
    path = _save_model(tmp_path / "model.npz")
    params = M.brisque_params(path)

    def run(**kw):
        torch.manual_seed(SEED)
        return evaluate_sequence(model, lr_dir, side, chunk=CHUNK, gumbel_uniform=noise, **kw)

    r_free = run(save_dir=str(tmp_path / "out"), brisque=path)                                # a path; no ground truth
    r_gt, r_gt_off = run(gt_dir=gt_dir, brisque=params), run(gt_dir=gt_dir)                    # a loaded model
    frames = np.stack([read_gray_png(str(tmp_path / "out" / ("%05d.png" % t))) for t in range(T)])
    assert frames.shape == (T, 4 * H, 4 * W)
    print("BRISQUE per frame:", " ".join("%.4f" % v for v in r_free.brisque))
    _check(r_gt, r_gt_off, r_free, frames, params, ("psnr", "ssim"), format_log)
    # NIQE and BRISQUE together: NIQE's figures are what they are alone, BRISQUE's too, and both suffixes stand in that order
    nq = M.niqe_params(niqe_ref.model())
    r_both, r_niqe = run(gt_dir=gt_dir, niqe=nq, brisque=params), run(gt_dir=gt_dir, niqe=nq)
    assert np.array_equal(r_both.brisque.view(np.uint64), r_gt.brisque.view(np.uint64))
    assert len(r_niqe.niqe) == T and np.array_equal(r_both.niqe.view(np.uint64), r_niqe.niqe.view(np.uint64))
    assert np.all(r_both.psnr == r_gt_off.psnr) and np.all(r_both.ssim == r_gt_off.ssim)
    assert format_log(r_niqe, "s") == format_log(r_gt_off, "s") + " NIQE: %.5f" % r_niqe.mean_niqe
    assert format_log(r_both, "s") == format_log(r_niqe, "s") + " BRISQUE: %.5f" % r_both.mean_brisque


def test_raw_yuv(model_and_noise, tmp_path):
    from cdfo_amd import metrics as M
    from cdfo_amd.evaluate import evaluate_yuv, format_log_yuv, write_synthetic_sequence_yuv
    from cdfo_amd.yuv import YuvReader
    model, noise = model_and_noise
    lr_yuv, side, gt_yuv = write_synthetic_sequence_yuv(str(tmp_path / "seq"), T, H, W, seed=11)
    params = M.brisque_params(ref.model())

    def run(**kw):
        torch.manual_seed(SEED)
        return evaluate_yuv(model, lr_yuv, W, H, side, chunk=CHUNK, gumbel_uniform=noise, **kw)

    r_free = run(save_yuv=str(tmp_path / "out.yuv"), brisque=ref.model())                      # the five arrays
    r_gt, r_gt_off = run(gt_yuv=gt_yuv, brisque=params), run(gt_yuv=gt_yuv)
    with YuvReader(str(tmp_path / "out.yuv"), 4 * W, 4 * H, "yuv420p") as f:
        assert f.frames == T
        frames = np.array(f.y(0, T))
    _check(r_gt, r_gt_off, r_free, frames, params, ("psnr_y", "psnr_u", "psnr_v", "ssim_y", "psnr_yuv"), format_log_yuv)


def test_refusals_before_any_launch(model_and_noise, tmp_path):
    from cdfo_amd.evaluate import (evaluate_sequence, evaluate_yuv, write_synthetic_sequence, write_synthetic_sequence_yuv)
    model, _ = model_and_noise
    lr_yuv, side, _ = write_synthetic_sequence_yuv(str(tmp_path / "ten"), 2, H, W, seed=3, gt=False, pix_fmt="yuv420p10le")
    with pytest.raises(ValueError, match="8-bit"):
        evaluate_yuv(model, lr_yuv, W, H, side, pix_fmt="yuv420p10le", brisque=ref.model())
    sv, coef, ranges, gamma, rho = ref.model()
    lr_dir, side, _ = write_synthetic_sequence(str(tmp_path / "seq"), 2, H, W, seed=3, gt=False)
    lr_yuv, side_yuv, _ = write_synthetic_sequence_yuv(str(tmp_path / "seq_yuv"), 2, H, W, seed=3, gt=False)
    flat = ranges.copy()
    flat[0, 1] = flat[0, 0]
    for bad in ((sv[:, :35], coef, ranges, gamma, rho), (sv, coef, flat, gamma, rho), (sv, coef * np.nan, ranges, gamma, rho)):
        with pytest.raises(ValueError):
            evaluate_sequence(model, lr_dir, side, brisque=bad)
        with pytest.raises(ValueError):
            evaluate_yuv(model, lr_yuv, W, H, side_yuv, brisque=bad)
    np.savez(tmp_path / "short.npz", sv=sv, sv_coef=coef)
    with pytest.raises(ValueError, match="feature_ranges"):
        evaluate_sequence(model, lr_dir, side, brisque=str(tmp_path / "short.npz"))
