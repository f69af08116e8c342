"""tOF without a device: the numpy statement of the definition (tests/tof_ref.py) against what the definition must yield, the host
pieces of `cdfo_amd.metrics` against the statement's, and every refusal of the option.

cv2 is not available, so nothing here pins parity with `cv2.calcOpticalFlowFarneback`; the checks are the definition's own: the stage
sizes (half-to-even in both directions), the polynomial expansion of an exact quadratic, the recovery of an integer translation of
a smooth 8-bit pattern (a sign or axis error gives at least the shift, 1 px and more; a correct statement measures below 6e-3 px, the
bound is 0.05 px), result == ground truth giving exactly 0, and the frame-0 rule being computed."""
import numpy as np
import pytest
import torch

import tof_ref as ref


def pattern(H: int, W: int, seed: int) -> np.ndarray:
    """uint8 [H,W]: a Gaussian-filtered (sigma 3) uniform random field scaled to 0 .. 255 and rounded."""
    x = np.random.RandomState(seed).rand(H, W)
    t = np.exp(-np.arange(-9.0, 10.0) ** 2 / (2.0 * 3.0 * 3.0))
    t /= t.sum()
    x = ref._taps_along(ref._taps_along(x, t, 0, ref._reflect101), t, 1, ref._reflect101)
    return np.rint((x - x.min()) / (x.max() - x.min()) * 255.0).astype(np.uint8)


def shifted_pair(H: int, W: int, sx: int, sy: int, seed: int = 1):
    """(prev, cur) cut from one canvas: cur(x, y) = prev(x - sx, y - sy), so the flow from prev to cur is (sx, sy)."""
    c = pattern(H + 32, W + 32, seed)
    return c[16:16 + H, 16:16 + W], c[16 - sy:16 - sy + H, 16 - sx:16 - sx + W]


@pytest.mark.parametrize("shape,want", [
    ((32, 32), [(0, 32, 32)]),
    ((33, 47), [(0, 33, 47)]),
    ((64, 80), [(1, 32, 40), (0, 64, 80)]),
    ((69, 131), [(1, 34, 66), (0, 69, 131)]),                               # 34.5 -> 34 and 65.5 -> 66: half to even, both ways
    ((136, 200), [(2, 34, 50), (1, 68, 100), (0, 136, 200)]),
    ((259, 301), [(3, 32, 38), (2, 65, 75), (1, 130, 150), (0, 259, 301)]),
    ((1080, 1920), [(3, 135, 240), (2, 270, 480), (1, 540, 960), (0, 1080, 1920)])])
def test_stage_sizes(shape, want):
    from cdfo_amd import metrics as M
    assert ref.levels(*shape) == want and M.tof_size(*shape) == want


def test_host_constants_are_the_statement_s():
    from cdfo_amd import metrics as M
    for k, n in ((0, 3), (1, 3), (2, 9), (3, 19)):
        assert len(ref.smooth_taps(k)) == n and np.array_equal(M.tof_taps(k), ref.smooth_taps(k))
        assert abs(ref.smooth_taps(k).sum() - 1.0) < 1e-15
    assert np.array_equal(ref.smooth_taps(0), [0.25, 0.5, 0.25])
    g, xg, xxg, *inv = ref.poly_kernels()
    assert np.array_equal(M.tof_poly_kernels(), np.concatenate([g, xg, xxg, inv]))
    assert abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1])


def test_polyexp_returns_the_coefficients_of_a_quadratic():
    h, w = 40, 50
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    c = (3.0, 0.5, -0.25, 0.01, -0.02, 0.015)
    got = ref.polyexp(c[0] + c[1] * x + c[2] * y + c[3] * x * x + c[4] * y * y + c[5] * x * y)
    want = [c[1] + 2 * c[3] * x + c[5] * y, c[2] + 2 * c[4] * y + c[5] * x, c[3] + 0 * x, c[4] + 0 * x, c[5] + 0 * x]
    inner = (slice(5, -5), slice(5, -5))
    worst = max(float(np.abs(got[i][inner] - want[i][inner]).max()) for i in range(5))
    print(f"polyexp of a quadratic: worst interior coefficient error {worst:.2e}")
    assert worst <= 1e-9


@pytest.mark.parametrize("H,W,sx,sy", [(64, 80, 2, -1), (259, 301, 5, -3)])
def test_translation_recovery(H, W, sx, sy):
    prev, cur = shifted_pair(H, W, sx, sy)
    f = ref.farneback(prev, cur)
    m = 20
    e = float(np.sqrt((f[m:-m, m:-m, 0] - sx) ** 2 + (f[m:-m, m:-m, 1] - sy) ** 2).mean())
    print(f"{H}x{W} shift ({sx},{sy}): interior mean endpoint error {e:.2e} px")
    assert f.shape == (H, W, 2) and e <= 0.05


def test_equal_stacks_give_exactly_zero_and_frame_0_is_computed():
    a, b = shifted_pair(64, 80, 2, -1, seed=5)
    gt = np.stack([a, b, a])
    assert np.array_equal(ref.tof(gt, gt.copy()), np.zeros(3))
    f0 = ref.farneback(a, a)                                    # an identical pair: not a zero flow (the last row and column always
    assert 0.0 < np.abs(f0).max() < 0.5                         # take the out-of-frame branch of the matrix update)
    sr = np.clip(gt.astype(np.int64) + np.random.RandomState(2).randint(-6, 7, gt.shape), 0, 255).astype(np.uint8)
    t = ref.tof(gt, sr)
    assert t.shape == (3,) and t[0] == ref.epe(ref.farneback(gt[0], gt[0]), ref.farneback(sr[0], sr[0])) and t[0] > 0.0
    assert np.all(t[1:] > 0.0) and np.all(np.isfinite(t))
    # the region is the common top-left rectangle
    assert np.array_equal(ref.tof(np.pad(gt, ((0, 0), (0, 3), (0, 5))), sr), t)


def test_result_fields_and_log_lines():
    from cdfo_amd import evaluate as E
    r = E.SequenceResult(np.array([30.0]), np.array([0.9]), 30.0, 0.9, 1, 0.5, 1.0)
    assert len(r.tof) == 0 and np.isnan(r.mean_tof) and E.format_log(r, "s") == "s Average PSNR/SSIM: 30.000/0.90000"
    r = r._replace(tof=np.array([0.125]), mean_tof=0.125)
    assert E.format_log(r, "s") == "s Average PSNR/SSIM: 30.000/0.90000 tOF: 0.12500"
    r = r._replace(brisque=np.array([61.5]), mean_brisque=61.5)
    assert E.format_log(r, "s").endswith(" BRISQUE: 61.50000 tOF: 0.12500")
    z = np.zeros(2)
    y = E.YuvResult(z, z, z, z, z, 31.0, 40.0, 41.0, 0.8, 33.375, 2, 0.5, 1.0)
    assert "tOF" not in E.format_log_yuv(y, "s") and len(y.tof) == 0 and np.isnan(y.mean_tof)
    assert E.format_log_yuv(y._replace(brisque=z, mean_brisque=7.0, tof=z, mean_tof=0.5), "s").endswith(" BRISQUE: 7.00000 tOF: 0.50000")


def test_every_refusal_needs_no_device(tmp_path):
    from cdfo_amd import evaluate as E
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M

    class Lr:
        dtype, peak, shape = torch.uint8, 255, (16, 20)

    class Lr10:
        dtype, peak, shape = torch.uint16, 1023, (16, 20)

    class Gt:
        shape = (64, 80)

    class GtSmall:
        shape = (31, 80)

    assert E._check_tof(Lr, None, False) is False and E._check_tof(Lr, Gt, True) is True
    with pytest.raises(ValueError, match="ground truth"):
        E._check_tof(Lr, None, True)
    with pytest.raises(ValueError, match="8-bit"):
        E._check_tof(Lr10, Gt, True)
    with pytest.raises(ValueError, match="32 x 32"):
        E._check_tof(Lr, GtSmall, True)
    # through the evaluators themselves: refused before the model is touched (None stands in for it)
    lr_dir, side, gt_dir = E.write_synthetic_sequence(str(tmp_path / "seq"), 2, 16, 20, seed=3)
    with pytest.raises(ValueError, match="ground truth"):
        E.evaluate_sequence(None, lr_dir, side, tof=True)
    lr_small, side_small, gt_small = E.write_synthetic_sequence(str(tmp_path / "small"), 2, 7, 20, seed=3)
    with pytest.raises(ValueError, match="32 x 32"):
        E.evaluate_sequence(None, lr_small, side_small, gt_dir=gt_small, tof=True)
    lr_yuv, side_yuv, gt_yuv = E.write_synthetic_sequence_yuv(str(tmp_path / "ten"), 2, 16, 20, seed=3, pix_fmt="yuv420p10le")
    with pytest.raises(ValueError, match="8-bit"):
        E.evaluate_yuv(None, lr_yuv, 20, 16, side_yuv, gt_yuv=gt_yuv, pix_fmt="yuv420p10le", tof=True)
    lr_yuv, side_yuv, _ = E.write_synthetic_sequence_yuv(str(tmp_path / "free"), 2, 16, 20, seed=3, gt=False)
    with pytest.raises(ValueError, match="ground truth"):
        E.evaluate_yuv(None, lr_yuv, 20, 16, side_yuv, tof=True)
    # the host functions and the wrappers
    u, d = torch.zeros((2, 32, 32), dtype=torch.uint8), torch.zeros((2, 5, 32, 32), dtype=torch.float64)
    bad = [lambda: M.tof_size(31, 32), lambda: M.tof_size(32, 31), lambda: M.tof_scratch(2, 31, 40, "cpu"),
           lambda: M.tof_scratch(0, 32, 32, "cpu"), lambda: M.farneback_u8(u, u), lambda: M.tof_frames_u8(u, u), lambda: M.tof_u8(u, u),
           lambda: K.tof_level(u, u, 32, 32, M.tof_taps(0)), lambda: K.tof_polyexp(d, M.tof_poly_kernels()),
           lambda: K.tof_matrices(d, None), lambda: K.tof_blur_solve(d), lambda: K.tof_flow_up(d, 64, 64), lambda: K.tof_epe(d, d)]
    for k, call in enumerate(bad):
        with pytest.raises((ValueError, NotImplementedError)):
            call()
            pytest.fail(f"call {k} did not raise")
