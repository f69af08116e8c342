"""evaluate_yuv at other pixel formats on the GPU (cdfo_amd/evaluate.py): T = 5 frames of 18x24 (padded to 24x24 inside), seeded
weights and injected noise, as tests/test_gpu_evaluate_yuv.py builds them.  The luma against `quantise_numpy` of the fp32 frames
`StreamingSR(peak=...)` returns under the same noise, the chroma against the reference filter, the figures against the helpers of
tests/pixfmt_ref.py on those integers; and the depth as such does not change what the model sees."""
import os

import numpy as np
import pytest
import torch

import pixfmt_ref

pytestmark = pytest.mark.gpu
T, H, W = 5, 18, 24
SEED = 4321
SSIM_TOL = 1e-9


@pytest.fixture(scope="module")
def model_and_noise():
    from arch.SIDECVSR_our import CVSR_V8
    from oracle.cvsr_v8_ref import make_inputs, make_state_dict
    m = CVSR_V8()
    m.load_state_dict(make_state_dict(21, perturb=True), strict=True)
    noise = [make_inputs(1, 24, 24, 900 + t)["gumbel_u"] for t in range(T)]
    return m.cuda().eval(), [[u.cuda() for u in six] for six in noise]


def _frames(model, noise, seq, peak, chunk):
    """fp32 [T,4H,4W] (numpy): what StreamingSR(peak=peak).run_chunked(chunk) returns for the arrays of `seq`."""
    from cdfo_amd.streaming import StreamingSR
    kw = dict(peak=peak) if peak != 255 else {}
    torch.manual_seed(SEED)
    s = StreamingSR(model, seq["lr"], seq["pms"], seq["rms"], seq["ufs"], seq["mvl0"], seq["mvl1"], gumbel_uniform=noise, **kw)
    return torch.cat(s.run_chunked(chunk))[:, 0].cpu().numpy()


def test_depth_does_not_change_what_the_model_sees(model_and_noise, tmp_path):
    """An 8-bit sequence, and the same with lr, rms and ufs multiplied by 257 at peak 65535 = 255 * 257: v / 255 and 257 v / 65535
    are correctly rounded fp32 quotients of one real number, so the planes, and with them the frames, are the same bits.
    Both objects divide by a device tensor: with a host scalar for a divisor torch's device kernel multiplies by the rounded
    reciprocal instead, which agrees with `v / 255` for 2207 of the 8000 integers in [-4000, 4000) only, and with which this identity
    missed by 6.67572e-06 in every frame."""
    from cdfo_amd.evaluate import write_synthetic_sequence_yuv
    from cdfo_amd.yuv import load_sequence_yuv
    model, noise = model_and_noise
    lr_yuv, side, _ = write_synthetic_sequence_yuv(str(tmp_path), T, H, W, seed=11, gt=False)
    seq = load_sequence_yuv(lr_yuv, W, H, side)
    wide = dict(seq, lr=seq["lr"].astype(np.uint16) * 257, rms=seq["rms"].astype(np.int32) * 257, ufs=seq["ufs"].astype(np.uint16) * 257)
    assert wide["lr"].max() > 60000 and wide["rms"].min() < -4000
    a, b = _frames(model, noise, seq, 255, 2), _frames(model, noise, wide, 65535, 2)
    assert a.shape == b.shape == (T, 4 * H, 4 * W) and a.dtype == np.float32
    print(f"max |difference| of the frames: {np.abs(a - b).max()!r}; frames differing: {int((a != b).any(axis=(1, 2)).sum())} of {T}")
    assert np.abs(a - b).max() == 0.0


@pytest.fixture(scope="module")
def ten_bit(model_and_noise, tmp_path_factory):
    """The yuv420p10le sequence on disk, its planes, and the expected frames per chunk size: made once, never changed."""
    from cdfo_amd.evaluate import quantise_numpy, write_synthetic_sequence_yuv
    from cdfo_amd.yuv import YuvReader, load_sequence_yuv
    model, noise = model_and_noise
    root = str(tmp_path_factory.mktemp("p10"))
    lr_yuv, side, gt_yuv = write_synthetic_sequence_yuv(root, T, H, W, seed=11, pix_fmt="yuv420p10le")
    seq = load_sequence_yuv(lr_yuv, W, H, side, "yuv420p10le")
    with YuvReader(gt_yuv, 4 * W, 4 * H, "yuv420p10le") as g:
        gt_y, gt_c = np.array(g.y(0, T)), np.stack([np.array(g.u(0, T)), np.array(g.v(0, T))])
    lr_c = np.stack([seq["u"], seq["v"]])                                    # [2,T,9,12]
    want_y = {chunk: quantise_numpy(_frames(model, noise, seq, 1023, chunk), peak=1023) for chunk in (2, 8)}
    assert want_y[2].dtype == np.uint16 and want_y[2].max() > 255
    return dict(files=(lr_yuv, side, gt_yuv), gt_y=gt_y, gt_c=gt_c, want_y=want_y, want_c=pixfmt_ref.up4(lr_c, 1023))


def _evaluate(model, noise, files, fmt, **kw):
    from cdfo_amd.evaluate import evaluate_yuv
    torch.manual_seed(SEED)
    return evaluate_yuv(model, files[0], W, H, files[1], gumbel_uniform=noise, **({} if fmt is None else dict(pix_fmt=fmt)), **kw)


@pytest.mark.parametrize("chunk", [2, 8])
def test_yuv420p10le_file_and_metrics(model_and_noise, ten_bit, chunk, tmp_path):
    """Chunk 2 (three chunks: every staging buffer is reused) and chunk 8 > T (one ragged chunk)."""
    from cdfo_amd.yuv import YuvReader
    model, noise = model_and_noise
    out = str(tmp_path / "out.yuv")
    r = _evaluate(model, noise, ten_bit["files"], "yuv420p10le", gt_yuv=ten_bit["files"][2], save_yuv=out, chunk=chunk)
    assert os.path.getsize(out) == T * 72 * 96 * 3 // 2 * 2
    with YuvReader(out, 4 * W, 4 * H, "yuv420p10le") as f:
        y, c = np.array(f.y(0, T)), np.stack([np.array(f.u(0, T)), np.array(f.v(0, T))])
    want_y, want_c = ten_bit["want_y"][chunk], ten_bit["want_c"]
    assert np.array_equal(y, want_y) and np.array_equal(c, want_c)
    assert r.psnr_y.dtype == np.float64 and r.psnr_y.shape == r.psnr_u.shape == r.psnr_v.shape == r.ssim_y.shape == (T,)
    for t in range(T):
        want_s = pixfmt_ref.calculate_ssim(want_y[t], ten_bit["gt_y"][t], 4, 1023)
        print(f"frame {t}: PSNR-Y {r.psnr_y[t]!r} U {r.psnr_u[t]!r} V {r.psnr_v[t]!r} SSIM-Y error {abs(r.ssim_y[t] - want_s):.2e}")
        assert r.psnr_y[t] == pixfmt_ref.calculate_psnr(want_y[t], ten_bit["gt_y"][t], 4, 1023)
        assert abs(r.ssim_y[t] - want_s) < SSIM_TOL
        for p, got in ((0, r.psnr_u), (1, r.psnr_v)):                       # numpy fp64 on the integers, chroma border 4 // 2
            d = want_c[p, t, 2:-2, 2:-2].astype(np.int64) - ten_bit["gt_c"][p, t, 2:-2, 2:-2].astype(np.int64)
            mse = (d * d).sum().astype(np.float64) / (32 * 44)
            assert got[t] == 20.0 * np.log10(1023.0 / np.sqrt(mse)) == pixfmt_ref.calculate_psnr(want_c[p, t], ten_bit["gt_c"][p, t], 2, 1023)
    assert np.array_equal(r.psnr_yuv, (6.0 * r.psnr_y + r.psnr_u + r.psnr_v) / 8.0)
    assert r.mean_psnr_y == r.psnr_y.sum() / T and r.mean_psnr_yuv == r.psnr_yuv.sum() / T and r.frames == T


def _other_format(model, noise, fmt, root):
    """(result, luma [T,72,96], chroma [2,T,.,.] or None, expected luma, ground truth reader planes) of a T-frame sequence at `fmt`."""
    from cdfo_amd.evaluate import quantise_numpy, write_synthetic_sequence_yuv
    from cdfo_amd.yuv import YuvReader, load_sequence_yuv
    files = write_synthetic_sequence_yuv(root, T, H, W, seed=11, pix_fmt=fmt)
    seq = load_sequence_yuv(files[0], W, H, files[1], fmt)
    want_y = quantise_numpy(_frames(model, noise, seq, 1023, 2), peak=1023)
    out = os.path.join(root, "out.yuv")
    r = _evaluate(model, noise, files, fmt, gt_yuv=files[2], save_yuv=out, chunk=2)
    gray = fmt.startswith("gray")
    with YuvReader(out, 4 * W, 4 * H, fmt) as f, YuvReader(files[2], 4 * W, 4 * H, fmt) as g:
        assert f.frames == T
        y, gy = np.array(f.y(0, T)), np.array(g.y(0, T))
        c = None if gray else np.stack([np.array(f.u(0, T)), np.array(f.v(0, T))])
        gc = None if gray else np.stack([np.array(g.u(0, T)), np.array(g.v(0, T))])
    assert np.array_equal(y, want_y)
    for t in range(T):
        assert r.psnr_y[t] == pixfmt_ref.calculate_psnr(want_y[t], gy[t], 4, 1023)
        assert abs(r.ssim_y[t] - pixfmt_ref.calculate_ssim(want_y[t], gy[t], 4, 1023)) < SSIM_TOL
    return r, seq, c, gc


def test_gray10le_has_no_chroma(model_and_noise, tmp_path):
    model, noise = model_and_noise
    r, seq, c, _ = _other_format(model, noise, "gray10le", str(tmp_path))
    assert os.path.getsize(str(tmp_path / "out.yuv")) == T * 72 * 96 * 2
    assert r.psnr_u.shape == r.psnr_v.shape == (0,) and np.isnan(r.mean_psnr_u) and np.isnan(r.mean_psnr_v)
    assert r.psnr_y.shape == (T,) and np.array_equal(r.psnr_yuv, r.psnr_y) and r.mean_psnr_yuv == r.mean_psnr_y


def test_yuv444p10le_chroma_has_the_lumas_size_and_border(model_and_noise, tmp_path):
    model, noise = model_and_noise
    r, seq, c, gc = _other_format(model, noise, "yuv444p10le", str(tmp_path))
    assert os.path.getsize(str(tmp_path / "out.yuv")) == T * 72 * 96 * 3 * 2
    want_c = pixfmt_ref.up4(np.stack([seq["u"], seq["v"]]), 1023)            # [2,T,72,96]
    assert c.shape == (2, T, 72, 96) and np.array_equal(c, want_c)
    for t in range(T):
        assert r.psnr_u[t] == pixfmt_ref.calculate_psnr(want_c[0, t], gc[0, t], 4, 1023)      # the border is crop_border itself
        assert r.psnr_v[t] == pixfmt_ref.calculate_psnr(want_c[1, t], gc[1, t], 4, 1023)
        assert r.psnr_u[t] != pixfmt_ref.calculate_psnr(want_c[0, t], gc[0, t], 2, 1023)
    assert np.array_equal(r.psnr_yuv, (6.0 * r.psnr_y + r.psnr_u + r.psnr_v) / 8.0)


def test_the_default_format_is_yuv420p(model_and_noise, tmp_path):
    """pix_fmt="yuv420p" returns the files and figures the call without the argument returns."""
    from cdfo_amd.evaluate import write_synthetic_sequence_yuv
    model, noise = model_and_noise
    files = write_synthetic_sequence_yuv(str(tmp_path / "raw"), T, H, W, seed=11)
    outs = [str(tmp_path / "a.yuv"), str(tmp_path / "b.yuv")]
    a = _evaluate(model, noise, files, None, gt_yuv=files[2], save_yuv=outs[0], chunk=2)
    b = _evaluate(model, noise, files, "yuv420p", gt_yuv=files[2], save_yuv=outs[1], chunk=2)
    assert open(outs[0], "rb").read() == open(outs[1], "rb").read() and os.path.getsize(outs[0]) == T * 72 * 96 * 3 // 2
    for name in ("psnr_y", "psnr_u", "psnr_v", "ssim_y", "psnr_yuv"):
        assert np.array_equal(getattr(a, name), getattr(b, name)) and getattr(a, name).shape == (T,)
    assert (a.mean_psnr_y, a.mean_ssim_y, a.mean_psnr_yuv) == (b.mean_psnr_y, b.mean_ssim_y, b.mean_psnr_yuv)
