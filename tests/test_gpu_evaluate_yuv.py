"""evaluate_yuv end to end on the GPU (cdfo_amd/evaluate.py): T = 5 frames of 18x24 (padded to 24x24 inside) in raw I420 files, ground
truth 72x96 with random chroma, seeded weights and injected noise.  The luma against what evaluate_sequence writes and reports for
the same content in the PNG layout, the chroma against the numpy statement of the filter (tests/chroma_ref.py) and numpy fp64."""
import os

import numpy as np
import pytest
import torch

from chroma_ref import up4

pytestmark = pytest.mark.gpu
T, H, W = 5, 18, 24
SEED = 4321


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """Model, the same content on disk in both layouts, and a cache of evaluate_sequence's results: made once, never changed."""
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd.evaluate import write_synthetic_sequence, write_synthetic_sequence_yuv
    from cdfo_amd.yuv import YuvReader
    from oracle.cvsr_v8_ref import make_inputs, make_state_dict
    root = str(tmp_path_factory.mktemp("yuv"))
    m = CVSR_V8()
    m.load_state_dict(make_state_dict(21, perturb=True), strict=True)
    lr_dir, side, gt_dir = write_synthetic_sequence(os.path.join(root, "png"), T, H, W, seed=11)
    lr_yuv, side_yuv, gt_yuv = write_synthetic_sequence_yuv(os.path.join(root, "raw"), T, H, W, seed=11)
    with YuvReader(lr_yuv, W, H) as r, YuvReader(gt_yuv, 4 * W, 4 * H) as g:
        lr_c = np.stack([np.array(r.u(0, T)), np.array(r.v(0, T))])          # [2,T,9,12]
        gt_c = np.stack([np.array(g.u(0, T)), np.array(g.v(0, T))])          # [2,T,36,48]
    noise = [make_inputs(1, 24, 24, 900 + t)["gumbel_u"] for t in range(T)]
    return dict(model=m.cuda().eval(), root=root, png=(lr_dir, side, gt_dir), raw=(lr_yuv, side_yuv, gt_yuv), lr_c=lr_c, gt_c=gt_c,
                want_c=up4(lr_c), step_noise=[[u.cuda() for u in six] for six in noise], frame_noise=[six[0].cuda() for six in noise],
                cache={})


def _noise(case, share):
    return dict(share_compensation=True, frame_noise=case["frame_noise"]) if share else dict(gumbel_uniform=case["step_noise"])


def _png_reference(case, chunk, share):
    """(result, frames [T,72,96]) of evaluate_sequence on the PNG layout of the same content, weights and noise."""
    from cdfo_amd.evaluate import evaluate_sequence
    from cdfo_amd.priors import read_gray_png
    if (chunk, share) not in case["cache"]:
        lr_dir, side, gt_dir = case["png"]
        save = os.path.join(case["root"], "ref_%d_%d" % (chunk, share))
        torch.manual_seed(SEED)
        r = evaluate_sequence(case["model"], lr_dir, side, gt_dir=gt_dir, save_dir=save, chunk=chunk, **_noise(case, share))
        case["cache"][(chunk, share)] = (r, np.stack([read_gray_png(os.path.join(save, "%05d.png" % t)) for t in range(T)]))
    return case["cache"][(chunk, share)]


def _evaluate(case, chunk, share, **kw):
    from cdfo_amd.evaluate import evaluate_yuv
    lr_yuv, side, _ = case["raw"]
    torch.manual_seed(SEED)
    return evaluate_yuv(case["model"], lr_yuv, W, H, side, chunk=chunk, **_noise(case, share), **kw)


def _read_i420(path):
    from cdfo_amd.yuv import YuvReader
    with YuvReader(path, 4 * W, 4 * H) as r:
        assert r.frames == T
        return np.array(r.y(0, T)), np.stack([np.array(r.u(0, T)), np.array(r.v(0, T))])


def _chroma_psnr(case):
    """numpy fp64 on the integers: mse over the common 36x48 less the chroma border 4 // 2, 20 log10(255 / sqrt(mse))."""
    d = case["want_c"][:, :, 2:-2, 2:-2].astype(np.int64) - case["gt_c"][:, :, 2:-2, 2:-2].astype(np.int64)
    sse = (d * d).sum(axis=(2, 3))
    assert sse.min() > 0
    mse = sse.astype(np.float64) / (32 * 44)
    return np.array([[20.0 * np.log10(255.0 / np.sqrt(m)) for m in row] for row in mse])


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("chunk", [2, 8])
def test_file_and_metrics(case, chunk, share, tmp_path):
    """Chunk 2 (three chunks: every staging buffer is reused) and chunk 8 > T (one ragged chunk); the default mode with per-step
    noise and the shared mode with per-frame noise."""
    from cdfo_amd.evaluate import format_log, format_log_yuv
    from oracle.metrics_ref import calculate_psnr
    ref, ref_frames = _png_reference(case, chunk, share)
    out = str(tmp_path / "out.yuv")
    r = _evaluate(case, chunk, share, gt_yuv=case["raw"][2], save_yuv=out)
    assert os.path.getsize(out) == T * 72 * 96 * 3 // 2
    y, c = _read_i420(out)
    assert np.array_equal(y, ref_frames)                                     # the luma: byte for byte evaluate_sequence's PNGs
    assert np.array_equal(c, case["want_c"])                                 # the chroma: the numpy statement on the LR chroma
    assert r.psnr_y.dtype == np.float64 and r.psnr_y.shape == r.psnr_u.shape == r.psnr_v.shape == r.ssim_y.shape == (T,)
    assert np.array_equal(r.psnr_y, ref.psnr) and np.array_equal(r.ssim_y, ref.ssim)
    want = _chroma_psnr(case)
    for t in range(T):
        print(f"frame {t}: PSNR-Y {r.psnr_y[t]!r} U {r.psnr_u[t]!r} ({want[0, t]!r}) V {r.psnr_v[t]!r} ({want[1, t]!r})")
        assert r.psnr_u[t] == want[0, t] == calculate_psnr(case["want_c"][0, t], case["gt_c"][0, t], 2)
        assert r.psnr_v[t] == want[1, t] == calculate_psnr(case["want_c"][1, t], case["gt_c"][1, t], 2)
    assert np.array_equal(r.psnr_yuv, (6.0 * r.psnr_y + r.psnr_u + r.psnr_v) / 8.0) and r.psnr_yuv.shape == (T,)
    for mean, a in ((r.mean_psnr_y, r.psnr_y), (r.mean_psnr_u, r.psnr_u), (r.mean_psnr_v, r.psnr_v), (r.mean_ssim_y, r.ssim_y),
                    (r.mean_psnr_yuv, r.psnr_yuv)):
        assert mean == a.sum() / T                                           # over the T frames
    assert r.mean_psnr_y == ref.mean_psnr and r.mean_ssim_y == ref.mean_ssim
    assert r.frames == T and 0 < r.seconds_forward < r.seconds_total
    assert format_log_yuv(r, "s").startswith(format_log(ref, "s") + " PSNR-U/V/YUV: %.3f/" % r.mean_psnr_u)


def test_without_ground_truth_and_without_saving(case, tmp_path):
    ref, ref_frames = _png_reference(case, 2, False)
    out = str(tmp_path / "out.yuv")
    r = _evaluate(case, 2, False, save_yuv=out)                              # frames, no metrics
    for a in (r.psnr_y, r.psnr_u, r.psnr_v, r.ssim_y, r.psnr_yuv):
        assert a.shape == (0,)
    assert all(np.isnan(m) for m in (r.mean_psnr_y, r.mean_psnr_u, r.mean_psnr_v, r.mean_ssim_y, r.mean_psnr_yuv)) and r.frames == T
    y, c = _read_i420(out)
    assert np.array_equal(y, ref_frames) and np.array_equal(c, case["want_c"])
    listing = sorted(os.listdir(os.path.join(case["root"], "raw")))
    r = _evaluate(case, 2, False, gt_yuv=case["raw"][2])                     # metrics, nothing written
    assert sorted(os.listdir(os.path.join(case["root"], "raw"))) == listing and sorted(os.listdir(str(tmp_path))) == ["out.yuv"]
    assert np.array_equal(r.psnr_y, ref.psnr) and np.array_equal(r.ssim_y, ref.ssim)
    want = _chroma_psnr(case)
    assert np.array_equal(r.psnr_u, want[0]) and np.array_equal(r.psnr_v, want[1])


def test_ground_truth_of_another_size_and_bad_files(case, tmp_path):
    """gt_size: a ground truth two rows taller and four columns narrower than the result is compared over the common size; a
    ground truth of another frame count, and a crop that leaves no window, are refused."""
    from cdfo_amd.yuv import YuvWriter
    from oracle.metrics_ref import calculate_psnr
    _, ref_frames = _png_reference(case, 2, False)
    rs = np.random.RandomState(9)
    gy, gu, gv = (rs.randint(0, 256, (T,) + s).astype(np.uint8) for s in ((74, 92), (37, 46), (37, 46)))
    other = str(tmp_path / "gt_92x74.yuv")
    with YuvWriter(other, 92, 74) as w:
        for t in range(T):
            w.append(gy[t], gu[t], gv[t])
    r = _evaluate(case, 2, False, gt_yuv=other, gt_size=(92, 74))
    for t in range(T):
        assert r.psnr_y[t] == calculate_psnr(ref_frames[t, :72, :92], gy[t, :72], 4)
        assert r.psnr_u[t] == calculate_psnr(case["want_c"][0, t, :36, :46], gu[t, :36], 2)
        assert r.psnr_v[t] == calculate_psnr(case["want_c"][1, t, :36, :46], gv[t, :36], 2)
    with pytest.raises(ValueError, match="frames"):
        _evaluate(case, 2, False, gt_yuv=other, gt_size=(46, 74))            # read as 10 frames of 46x74
    with pytest.raises(ValueError, match="SSIM window"):
        _evaluate(case, 2, False, gt_yuv=case["raw"][2], crop_border=32)


def test_gray_raw_file_is_the_png_path(case, tmp_path):
    """One loop, two front ends: the same luma as a `gray` raw file through evaluate_yuv and as PNGs through evaluate_sequence
    (chunk 2: every staging buffer is reused) give the same bytes and the same figures."""
    from cdfo_amd.evaluate import evaluate_yuv, write_synthetic_sequence_yuv
    from cdfo_amd.yuv import YuvReader
    ref, ref_frames = _png_reference(case, 2, False)
    lr_yuv, side, gt_yuv = write_synthetic_sequence_yuv(str(tmp_path / "gray"), T, H, W, seed=11, pix_fmt="gray")
    out = str(tmp_path / "out.yuv")
    torch.manual_seed(SEED)
    r = evaluate_yuv(case["model"], lr_yuv, W, H, side, gt_yuv=gt_yuv, save_yuv=out, chunk=2, pix_fmt="gray", **_noise(case, False))
    with YuvReader(out, 4 * W, 4 * H, "gray") as saved:
        assert saved.frames == T and np.array_equal(saved.y(0, T), ref_frames)
    assert np.array_equal(r.psnr_y, ref.psnr) and np.array_equal(r.ssim_y, ref.ssim) and r.psnr_y.shape == (T,)
    assert r.psnr_u.shape == r.psnr_v.shape == (0,)
    assert r.psnr_yuv is r.psnr_y
