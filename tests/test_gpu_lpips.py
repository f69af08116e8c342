"""LPIPS end to end on the GPU: `metrics.lpips_layers_u8` / `lpips_u8` against the fp64 statement (tests/lpips_ref.py), and ``lpips=``
in both evaluators.

Against the statement (tests/lpips_cases.py): a narrow net (widths 16, 32, 48, 64, 64) at 16 x 16 and 37 x 53 with three frames, the
true widths once at 32 x 32, and a 40 x 64 result against a 37 x 70 ground truth (the common region 37 x 64, both read in place).  The
device's trunk is fp32, the statement's fp64, so the bound is the fp32 floor: per layer 16 x the worst relative distance of the
statement's own fp32-trunk form from its fp64 form over these cases, and for the total 16 x the worst such distance of the totals --
both measured on the CPU when the test runs, from the statement alone.  The margin covers the matrix cores' accumulation order
against ATen's; a wrong tap, pool phase, channel weight or a missing border term moves a layer by 1e-2 or more.  Measured on one
MI355X: per layer 7.88e-6 at worst and 2.69e-7 on the total, where the floors were 8.75e-6 and 3.32e-7 (DESIGN.md has every case).

Evaluators: T = 5 frames of 18 x 24 (a 72 x 96 result) at chunk 2 and at chunk 8; T is no multiple of 2, and the bits must be those of
`lpips_u8` on the saved frames."""
import numpy as np
import pytest
import torch

import lpips_cases as cases
import lpips_ref as ref

pytestmark = pytest.mark.gpu
T, H, W = 5, 18, 24
SEED = 4321


@pytest.mark.parametrize("name", list(cases.CASES))
def test_layers_match_the_statement(name):
    from cdfo_amd import metrics as M
    params, sr, gt, want, _ = cases.case(name)
    floor_layer, floor_total = cases.floors()
    dsr, dgt = torch.from_numpy(np.array(sr)).cuda(), torch.from_numpy(np.array(gt)).cuda()
    layers = M.lpips_layers_u8(dsr, dgt, params)
    assert layers.shape == (len(sr), 5) and layers.dtype == torch.float64 and layers.is_cuda
    got = layers.cpu().numpy()
    err, err_total = cases.rel(got, want), cases.rel(cases.totals(got), cases.totals(want))
    print(f"{name}: device against the fp64 statement: per layer {err:.2e} (floor {floor_layer:.2e}), total {err_total:.2e} "
          f"(floor {floor_total:.2e}); LPIPS {M.lpips_from_layers(got)}")
    assert np.isfinite(got).all() and err <= 16 * floor_layer and err_total <= 16 * floor_total
    total = M.lpips_u8(dsr, dgt, params)
    assert total.shape == (len(sr),) and total.dtype == np.float64
    assert np.array_equal(total.view(np.uint64), cases.totals(got).view(np.uint64))
    assert np.array_equal(M.lpips_u8(dsr, dsr.clone(), params), np.zeros(len(sr)))           # result == ground truth: exactly 0
    assert np.array_equal(M.lpips_u8(dgt, dsr, params).view(np.uint64), total.view(np.uint64))          # symmetric, bit for bit


def test_normalize_false_matches_the_statement_and_differs():
    from cdfo_amd import metrics as M
    params, sr, gt, want_on, _ = cases.case("narrow-37x53")
    floor_layer, _ = cases.floors()
    want = np.stack([ref.layers(sr[j], gt[j], params, normalize=False) for j in range(len(sr))])
    got = M.lpips_layers_u8(torch.from_numpy(np.array(sr)).cuda(), torch.from_numpy(np.array(gt)).cuda(), params, normalize=False).cpu().numpy()
    print(f"normalize=False: per layer {cases.rel(got, want):.2e}; against the default's statement {cases.rel(got, want_on):.2e}")
    assert cases.rel(got, want) <= 16 * floor_layer and cases.rel(got, want_on) > 1e-3


def test_pairs_per_pass_do_not_move_a_bit():
    from cdfo_amd import metrics as M
    params, sr, gt, _, _ = cases.case("narrow-37x53")
    dsr, dgt = torch.from_numpy(np.array(sr)).cuda(), torch.from_numpy(np.array(gt)).cuda()
    one = M.lpips_layers_u8(dsr, dgt, params, M.lpips_scratch(3, 37, 53, params, "cuda", pairs=1)).cpu().numpy()
    for pairs in (2, 3, 4):
        scratch = M.lpips_scratch(4, 37, 53, params.widths, "cuda", pairs=pairs)
        assert scratch.nbytes == M.LpipsScratch.bytes_for(pairs, 37, 53, params.widths, 4)
        many = M.lpips_layers_u8(dsr, dgt, params, scratch).cpu().numpy()
        assert np.array_equal(one.view(np.uint64), many.view(np.uint64)), pairs
    with pytest.raises(ValueError, match="scratch"):
        M.lpips_layers_u8(dsr, dgt, params, M.lpips_scratch(2, 37, 53, params, "cuda"))       # a scratch for two frames, three given
    with pytest.raises(ValueError, match="scratch"):
        M.lpips_layers_u8(dsr, dgt, params, M.lpips_scratch(3, 37, 52, params, "cuda"))
    with pytest.raises(ValueError, match="16 x 16"):
        M.lpips_layers_u8(dsr[:, :15], dgt, params)


@pytest.fixture(scope="module")
def model_and_noise():
    from arch.SIDECVSR_our import CVSR_V8
    from oracle.cvsr_v8_ref import make_inputs, make_state_dict
    m = CVSR_V8()
    m.load_state_dict(make_state_dict(21, perturb=True), strict=True)
    noise = [make_inputs(1, 24, 24, 900 + t)["gumbel_u"] for t in range(T)]          # at the padded LR size
    return m.cuda().eval(), [[u.cuda() for u in six] for six in noise]


def _check(r2, r8, r_off, r_plain, frames, gt, names, log, params):
    from cdfo_amd import metrics as M
    for r in (r2, r8):
        assert r.lpips.dtype == np.float64 and r.lpips.shape == (T,) and np.isfinite(r.lpips).all() and np.all(r.lpips > 0.0)
        assert r.mean_lpips == r.lpips.sum() / T
    assert np.array_equal(r2.lpips.view(np.uint64), r8.lpips.view(np.uint64))               # the chunk size does not move a bit
    want = M.lpips_u8(torch.from_numpy(frames).cuda(), torch.from_numpy(gt).cuda(), params)
    assert np.array_equal(r8.lpips.view(np.uint64), want.view(np.uint64))
    print("LPIPS per frame:", r8.lpips)
    for r in (r_off, r_plain):
        assert len(r.lpips) == 0 and np.isnan(r.mean_lpips)
    assert log(r_off, "s") == log(r_plain, "s") and "LPIPS" not in log(r_off, "s")          # lpips=None: the line of a call without it
    assert log(r8, "s") == log(r_off, "s") + " LPIPS: %.5f" % r8.mean_lpips
    for name in names:                                                                      # the other figures do not move, bit for bit
        x, y, z = getattr(r8, name), getattr(r_plain, name), getattr(r_off, name)
        assert len(x) == T and x.shape == y.shape and np.all(x == y) and np.all(z == y), name
    for name in r_plain._fields:                                                            # option off: every field a call without it has
        x, y = getattr(r_off, name), getattr(r_plain, name)
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True), name
        elif "seconds" not in name:
            assert x == y or (x != x and y != y), name


def test_png_directories(model_and_noise, tmp_path):
    from cdfo_amd.evaluate import evaluate_sequence, format_log, write_synthetic_sequence
    from cdfo_amd.priors import read_gray_png
    model, noise = model_and_noise
    params = cases.model(cases.NARROW, 11)
    lr_dir, side, gt_dir = write_synthetic_sequence(str(tmp_path / "seq"), T, H, W, seed=11)

    def run(**kw):
        torch.manual_seed(SEED)
        return evaluate_sequence(model, lr_dir, side, gt_dir=gt_dir, gumbel_uniform=noise, **kw)

    r2, r8 = run(chunk=2, lpips=params), run(chunk=8, lpips=params.arrays(), save_dir=str(tmp_path / "out"))
    r_off, r_plain = run(chunk=8, lpips=None), run(chunk=8)
    frames = np.stack([read_gray_png(str(tmp_path / "out" / ("%05d.png" % t))) for t in range(T)])
    gt = np.stack([read_gray_png(str(tmp_path / "seq" / "gt" / ("%05d.png" % t))) for t in range(T)])
    assert frames.shape == (T, 4 * H, 4 * W) and gt.shape == frames.shape
    _check(r2, r8, r_off, r_plain, frames, gt, ("psnr", "ssim"), format_log, params)


def test_raw_yuv(model_and_noise, tmp_path):
    from cdfo_amd.evaluate import evaluate_yuv, format_log_yuv, write_synthetic_sequence_yuv
    from cdfo_amd.yuv import YuvReader
    model, noise = model_and_noise
    params = cases.model(cases.NARROW, 11)
    np.savez(tmp_path / "model.npz", **params.arrays())
    lr_yuv, side, gt_yuv = write_synthetic_sequence_yuv(str(tmp_path / "seq"), T, H, W, seed=11)

    def run(**kw):
        torch.manual_seed(SEED)
        return evaluate_yuv(model, lr_yuv, W, H, side, gt_yuv=gt_yuv, gumbel_uniform=noise, **kw)

    r2, r8 = run(chunk=2, lpips=str(tmp_path / "model.npz")), run(chunk=8, lpips=params, save_yuv=str(tmp_path / "out.yuv"))
    r_off, r_plain = run(chunk=8, lpips=None), run(chunk=8)
    with YuvReader(str(tmp_path / "out.yuv"), 4 * W, 4 * H, "yuv420p") as f:
        frames = np.array(f.y(0, T))
    with YuvReader(gt_yuv, 4 * W, 4 * H, "yuv420p") as f:
        gt = np.array(f.y(0, T))
    _check(r2, r8, r_off, r_plain, frames, gt, ("psnr_y", "psnr_u", "psnr_v", "ssim_y", "psnr_yuv"), format_log_yuv, params)


def test_refusals_before_any_launch(model_and_noise, tmp_path):
    from cdfo_amd.evaluate import evaluate_sequence, evaluate_yuv, write_synthetic_sequence, write_synthetic_sequence_yuv
    model, _ = model_and_noise
    params = cases.model(cases.NARROW, 11)
    lr_yuv, side, gt_yuv = write_synthetic_sequence_yuv(str(tmp_path / "ten"), 2, H, W, seed=3, pix_fmt="yuv420p10le")
    with pytest.raises(ValueError, match="8-bit"):
        evaluate_yuv(model, lr_yuv, W, H, side, gt_yuv=gt_yuv, pix_fmt="yuv420p10le", lpips=params)
    lr_dir, side, _ = write_synthetic_sequence(str(tmp_path / "seq"), 2, H, W, seed=3, gt=False)
    with pytest.raises(ValueError, match="ground truth"):
        evaluate_sequence(model, lr_dir, side, lpips=params)
    lr_dir, side, gt_dir = write_synthetic_sequence(str(tmp_path / "seq2"), 2, H, W, seed=3)
    with pytest.raises(ValueError, match="LPIPS model"):
        evaluate_sequence(model, lr_dir, side, gt_dir=gt_dir, lpips={"w0": np.zeros((16, 3, 3, 3))})
