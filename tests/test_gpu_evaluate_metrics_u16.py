"""``evaluate_yuv(..., rescale_metrics=True)`` on the GPU: NIQE, BRISQUE, tOF and LPIPS of a high-bit-depth sequence.

A yuv420p10le sequence of T = 3 frames of 24 x 32 (a 96 x 128 result: one row of NIQE blocks), seeded weights and injected noise as
tests/test_gpu_evaluate_pixfmt.py builds them.  At chunk 2 the second chunk holds one frame, so tOF's carried pair crosses a chunk.
The four scores must be the bits of `metrics.niqe_u16`, `brisque_u16`, `tof_u16` and `lpips_u16` on the frames read back from the
result file (LPIPS too: the evaluator's scratch takes one pair per pass, as `lpips_u16`'s own does, so the trunk calls are the same);
chunks of 1 and of 3 give those bits again; without the keyword the call still raises; the other figures are those of a call with no
such metric; one gray12le run without ground truth; and an 8-bit format with the keyword gives the bits of the call without it."""
import numpy as np
import pytest
import torch

import brisque_ref
import lpips_cases
import niqe_ref

pytestmark = pytest.mark.gpu
T, H, W = 3, 24, 32
SEED = 4321
FOUR = ("niqe", "brisque", "tof", "lpips")


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def model_and_noise():
    from arch.SIDECVSR_our import CVSR_V8
    from oracle.cvsr_v8_ref import make_inputs, make_state_dict
    m = CVSR_V8()
    m.load_state_dict(make_state_dict(21, perturb=True), strict=True)
    noise = [make_inputs(1, H, W, 900 + t)["gumbel_u"] for t in range(T)]
    return m.cuda().eval(), [[u.cuda() for u in six] for six in noise]


@pytest.fixture(scope="module")
def models():
    return dict(niqe=niqe_ref.model(), brisque=brisque_ref.model(), tof=True, lpips=lpips_cases.model(lpips_cases.NARROW, 11))


def _run(model_and_noise, files, fmt, **kw):
    from cdfo_amd.evaluate import evaluate_yuv
    model, noise = model_and_noise
    torch.manual_seed(SEED)
    return evaluate_yuv(model, files[0], W, H, files[1], gt_yuv=files[2], gumbel_uniform=noise, pix_fmt=fmt, **kw)


@pytest.fixture(scope="module")
def ten_bit(model_and_noise, models, tmp_path_factory):
    """The sequence, the run at chunk 2 with the result saved, and the frames read back: made once, never changed."""
    from cdfo_amd.evaluate import write_synthetic_sequence_yuv
    from cdfo_amd.yuv import YuvReader
    root = tmp_path_factory.mktemp("p10")
    files = write_synthetic_sequence_yuv(str(root / "seq"), T, H, W, seed=11, pix_fmt="yuv420p10le")
    out = str(root / "out.yuv")
    r = _run(model_and_noise, files, "yuv420p10le", chunk=2, rescale_metrics=True, save_yuv=out, **models)
    with YuvReader(out, 4 * W, 4 * H, "yuv420p10le") as f:
        sr = np.array(f.y(0, T))
    with YuvReader(files[2], 4 * W, 4 * H, "yuv420p10le") as f:
        gt = np.array(f.y(0, T))
    assert sr.dtype == np.uint16 and sr.shape == gt.shape == (T, 4 * H, 4 * W) and 255 < sr.max() <= 1023
    return dict(files=files, r=r, sr=sr, gt=gt)


def test_scores_are_those_of_the_u16_functions_on_the_saved_frames(ten_bit, models):
    from cdfo_amd import metrics as M
    from cdfo_amd.evaluate import format_log_yuv
    r = ten_bit["r"]
    sr, gt = torch.from_numpy(ten_bit["sr"]).cuda(), torch.from_numpy(ten_bit["gt"]).cuda()
    want = dict(niqe=M.niqe_u16(sr, 1023, models["niqe"]), brisque=M.brisque_u16(sr, 1023, models["brisque"]),
                tof=M.tof_u16(gt, sr, 1023), lpips=M.lpips_u16(sr, gt, 1023, models["lpips"]))
    for name in FOUR:
        got = getattr(r, name)
        print(f"{name}: {got}")
        assert got.dtype == np.float64 and got.shape == (T,) and np.isfinite(got).all(), name
        assert np.array_equal(bits(got), bits(want[name])), name
        assert getattr(r, "mean_" + name) == got.sum() / T
    assert np.all(r.tof > 0.0) and np.all(r.lpips > 0.0)
    assert format_log_yuv(r, "s").endswith(" NIQE: %.5f BRISQUE: %.5f tOF: %.5f LPIPS: %.5f" % (r.mean_niqe, r.mean_brisque, r.mean_tof, r.mean_lpips))


@pytest.mark.parametrize("chunk", [1, 3])
def test_the_chunk_size_does_not_move_a_bit(model_and_noise, models, ten_bit, chunk):
    r = _run(model_and_noise, ten_bit["files"], "yuv420p10le", chunk=chunk, rescale_metrics=True, **models)
    for name in FOUR:
        assert np.array_equal(bits(getattr(r, name)), bits(getattr(ten_bit["r"], name))), name


def test_without_the_keyword_the_call_raises_and_the_other_figures_do_not_move(model_and_noise, models, ten_bit):
    for name in FOUR:
        with pytest.raises(ValueError, match="8-bit"):
            _run(model_and_noise, ten_bit["files"], "yuv420p10le", chunk=2, **{name: models[name]})
        with pytest.raises(ValueError, match="8-bit"):
            _run(model_and_noise, ten_bit["files"], "yuv420p10le", chunk=2, rescale_metrics=False, **{name: models[name]})
    plain, r = _run(model_and_noise, ten_bit["files"], "yuv420p10le", chunk=2), ten_bit["r"]
    keyed = _run(model_and_noise, ten_bit["files"], "yuv420p10le", chunk=2, rescale_metrics=True)       # the keyword alone: nothing runs
    for name in ("psnr_y", "psnr_u", "psnr_v", "ssim_y", "psnr_yuv", "msssim"):
        assert np.array_equal(bits(getattr(r, name)), bits(getattr(plain, name))), name
    for name in plain._fields:
        x, y = getattr(keyed, name), getattr(plain, name)
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), name
        elif "seconds" not in name:
            assert x == y or (x != x and y != y), name


def test_gray12le_without_ground_truth(model_and_noise, models, tmp_path):
    from cdfo_amd import metrics as M
    from cdfo_amd.evaluate import evaluate_yuv, write_synthetic_sequence_yuv
    from cdfo_amd.yuv import YuvReader
    model, noise = model_and_noise
    lr, side, _ = write_synthetic_sequence_yuv(str(tmp_path / "seq"), T, H, W, seed=12, gt=False, pix_fmt="gray12le")
    out = str(tmp_path / "out.yuv")
    torch.manual_seed(SEED)
    r = evaluate_yuv(model, lr, W, H, side, gumbel_uniform=noise, pix_fmt="gray12le", chunk=2, rescale_metrics=True, save_yuv=out,
                     niqe=models["niqe"], brisque=models["brisque"])
    with YuvReader(out, 4 * W, 4 * H, "gray12le") as f:
        frames = np.array(f.y(0, T))
    assert frames.dtype == np.uint16 and 255 < frames.max() <= 4095
    sr = torch.from_numpy(frames).cuda()
    assert np.array_equal(bits(r.niqe), bits(M.niqe_u16(sr, 4095, models["niqe"]))) and np.isfinite(r.niqe).all()
    assert np.array_equal(bits(r.brisque), bits(M.brisque_u16(sr, 4095, models["brisque"]))) and np.isfinite(r.brisque).all()
    assert len(r.psnr_y) == len(r.tof) == len(r.lpips) == 0
    with pytest.raises(ValueError, match="ground truth"):
        evaluate_yuv(model, lr, W, H, side, pix_fmt="gray12le", rescale_metrics=True, tof=True)


def test_an_8_bit_format_with_the_keyword_gives_the_bits_of_the_call_without_it(model_and_noise, models, tmp_path):
    from cdfo_amd.evaluate import write_synthetic_sequence_yuv
    files = write_synthetic_sequence_yuv(str(tmp_path / "seq"), T, H, W, seed=11)
    off = _run(model_and_noise, files, "yuv420p", chunk=2, **models)
    on = _run(model_and_noise, files, "yuv420p", chunk=2, rescale_metrics=True, **models)
    for name in off._fields:
        x, y = getattr(on, name), getattr(off, name)
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), name
            assert len(x) == (0 if name == "msssim" else T), name
        elif "seconds" not in name:
            assert x == y or (x != x and y != y), name
