"""NIQE, BRISQUE, tOF and LPIPS above 8 bits, the parts that need no device (DESIGN.md has the definition, the project's own).

A 16-bit sample v of a format with the peak P becomes x = (255 v) / P in fp64 for NIQE, BRISQUE and tOF -- an exact product and one
correctly rounded division -- and x01 = (float)v / (float)P in fp32 for LPIPS' stem.  Checked here in numpy: v = 257 k at the peak
65535 gives x = k exactly and x01 the bits of (float)k / 255.f for every k in 0 .. 255, so the statements of the three fp64 metrics fed
such frames give what they give on the 8-bit frames k; the evaluators' checks let a uint16 source through with ``rescale_metrics``
only, and keep the order of their errors; the ``_u16`` wrappers refuse a wrong dtype, peak or shape before they touch the library."""
import numpy as np
import pytest
import torch

import brisque_ref
import niqe_ref
import tof_ref
from test_tof_cpu import shifted_pair

K8 = np.arange(256)


def scaled(u8: np.ndarray, peak: int = 65535) -> np.ndarray:
    """The fp64 samples the 16-bit kernels form of the uint16 frame u8 * (peak // 255): (255 v) / peak."""
    v = (u8.astype(np.uint16) * np.uint16(peak // 255)).astype(np.float64)
    return (255.0 * v) / float(peak)


def test_scaling_identities():
    v = (257 * K8).astype(np.uint16)
    assert v[-1] == 65535
    x = (255.0 * v.astype(np.float64)) / 65535.0
    assert np.array_equal(x, K8.astype(np.float64))
    x01 = v.astype(np.float32) / np.float32(65535.0)
    want = K8.astype(np.float32) / np.float32(255.0)
    assert x01.dtype == np.float32 and np.array_equal(x01.view(np.uint32), want.view(np.uint32))
    # the product is exact at every peak and sample: 255 * 65535 < 2^24
    for peak in (1023, 4095, 65535):
        s = np.arange(peak + 1, dtype=np.int64)
        assert np.array_equal((255.0 * s.astype(np.float64)).astype(np.int64), 255 * s)
    # a reciprocal is NOT the quotient: at least one 10-bit sample differs, which is why the kernels divide
    s = np.arange(1024, dtype=np.float64)
    assert ((255.0 * s) * (1.0 / 1023.0) != (255.0 * s) / 1023.0).any()


def test_statements_on_scaled_frames_equal_themselves_on_u8():
    rs = np.random.RandomState(5)
    u = rs.randint(0, 256, (100, 197)).astype(np.uint8)
    assert np.array_equal(scaled(u), u.astype(np.float64))
    a, b = niqe_ref.pieces(scaled(u)), niqe_ref.pieces(u)
    for key in ("mscn1", "half", "mscn2", "sums1", "sums2", "features"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert np.array_equal(niqe_ref.features(scaled(u)), niqe_ref.features(u), equal_nan=True)
    u = rs.randint(0, 256, (37, 83)).astype(np.uint8)
    a, b = brisque_ref.pieces(scaled(u)), brisque_ref.pieces(u)
    for key in ("mscn1", "half", "mscn2", "features"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    p, c = shifted_pair(37, 45, 2, -1, seed=3)
    for k, h, w in tof_ref.levels(37, 45):
        assert np.array_equal(tof_ref.level_image(scaled(p), k, h, w), tof_ref.level_image(p, k, h, w))
    assert np.array_equal(tof_ref.farneback(scaled(p), scaled(c)), tof_ref.farneback(p, c))


class Lr:
    dtype, peak, shape = torch.uint8, 255, (24, 32)


class Lr10:
    dtype, peak, shape = torch.uint16, 1023, (24, 32)


class Lr10Small:
    dtype, peak, shape = torch.uint16, 1023, (3, 32)


class Gt:
    shape = (96, 128)


class GtSmall:
    shape = (15, 128)


def _models():
    from cdfo_amd import metrics as M
    return (M.niqe_params(niqe_ref.model()), M.brisque_params(brisque_ref.model()),
            M.lpips_random_params((16, 32, 48, 64, 64), 0))


def test_checks_without_the_keyword_still_refuse_16_bit_sources():
    from cdfo_amd import evaluate as E
    nq, bq, lp = _models()
    for call in (lambda **kw: E._check_niqe(Lr10, nq, **kw), lambda **kw: E._check_brisque(Lr10, bq, **kw),
                 lambda **kw: E._check_tof(Lr10, Gt, True, **kw), lambda **kw: E._check_lpips(Lr10, Gt, lp, **kw)):
        with pytest.raises(ValueError, match="8-bit"):
            call()
        with pytest.raises(ValueError, match="8-bit"):
            call(rescale_metrics=False)


def test_checks_with_the_keyword_pass_and_keep_their_other_errors():
    from cdfo_amd import evaluate as E
    from cdfo_amd import metrics as M
    nq, bq, lp = _models()
    for lr in (Lr, Lr10):
        assert E._check_niqe(lr, nq, rescale_metrics=True) is nq and E._check_brisque(lr, bq, rescale_metrics=True) is bq
        assert E._check_tof(lr, Gt, True, rescale_metrics=True) is True
        assert isinstance(E._check_lpips(lr, Gt, lp, rescale_metrics=True), M.LpipsParams)
        # off stays off
        assert E._check_niqe(lr, None, True) is None and E._check_brisque(lr, None, True) is None
        assert E._check_tof(lr, Gt, False, True) is False and E._check_lpips(lr, Gt, None, True) is None
    # the size limits
    with pytest.raises(ValueError, match="96 x 96"):
        E._check_niqe(Lr10Small, nq, rescale_metrics=True)
    with pytest.raises(ValueError, match="16 x 16"):
        E._check_brisque(Lr10Small, bq, rescale_metrics=True)
    with pytest.raises(ValueError, match="32 x 32"):
        E._check_tof(Lr10, GtSmall, True, rescale_metrics=True)
    with pytest.raises(ValueError, match="16 x 16"):
        E._check_lpips(Lr10, GtSmall, lp, rescale_metrics=True)
    # the existing order: no ground truth comes before the depth and the size, a bad model before everything
    with pytest.raises(ValueError, match="ground truth"):
        E._check_tof(Lr10, None, True, rescale_metrics=True)
    with pytest.raises(ValueError, match="ground truth"):
        E._check_lpips(Lr10, None, lp, rescale_metrics=True)
    with pytest.raises(ValueError, match="ground truth"):
        E._check_tof(Lr10, None, True)
    with pytest.raises(ValueError):
        E._check_niqe(Lr10Small, (np.zeros(35), np.zeros((36, 36))), rescale_metrics=True)


def test_evaluators_take_the_keyword_before_the_model(tmp_path):
    """None stands in for the model: every refusal comes before it is touched."""
    from cdfo_amd import evaluate as E
    nq, bq, lp = _models()
    lr, side, gt = E.write_synthetic_sequence_yuv(str(tmp_path / "ten"), 2, 8, 12, seed=3, pix_fmt="yuv420p10le")
    for kw in (dict(niqe=nq), dict(brisque=bq), dict(tof=True), dict(lpips=lp)):
        with pytest.raises(ValueError, match="8-bit"):
            E.evaluate_yuv(None, lr, 12, 8, side, gt_yuv=gt, pix_fmt="yuv420p10le", **kw)
    # with the keyword the 32 x 48 frames get as far as the size limits
    with pytest.raises(ValueError, match="96 x 96"):
        E.evaluate_yuv(None, lr, 12, 8, side, gt_yuv=gt, pix_fmt="yuv420p10le", niqe=nq, rescale_metrics=True)
    lr, side, gt = E.write_synthetic_sequence_yuv(str(tmp_path / "small"), 2, 2, 12, seed=3, pix_fmt="yuv420p10le")
    with pytest.raises(ValueError, match="16 x 16"):
        E.evaluate_yuv(None, lr, 12, 2, side, gt_yuv=gt, pix_fmt="yuv420p10le", rescale_metrics=True, brisque=bq)
    mid = E.write_synthetic_sequence_yuv(str(tmp_path / "mid"), 2, 6, 12, seed=3, pix_fmt="yuv420p10le")     # 24 x 48: SSIM fits, tOF not
    with pytest.raises(ValueError, match="32 x 32"):
        E.evaluate_yuv(None, mid[0], 12, 6, mid[1], gt_yuv=mid[2], pix_fmt="yuv420p10le", rescale_metrics=True, tof=True)
    for kw in (dict(tof=True), dict(lpips=lp)):
        with pytest.raises(ValueError, match="ground truth"):
            E.evaluate_yuv(None, lr, 12, 2, side, pix_fmt="yuv420p10le", rescale_metrics=True, **kw)
    # evaluate_sequence accepts it too: its refusals are the ones it had
    lr_dir, side, gt_dir = E.write_synthetic_sequence(str(tmp_path / "png"), 2, 8, 12, seed=3)
    with pytest.raises(ValueError, match="96 x 96"):
        E.evaluate_sequence(None, lr_dir, side, gt_dir=gt_dir, niqe=nq, rescale_metrics=True)
    with pytest.raises(ValueError, match="ground truth"):
        E.evaluate_sequence(None, lr_dir, side, tof=True, rescale_metrics=True)


def test_wrapper_argument_errors_come_before_any_library_call(monkeypatch):
    from cdfo_amd import _lib
    from cdfo_amd import metrics as M

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    nq, bq, lp = _models()
    u16 = torch.zeros((2, 96, 128), dtype=torch.uint16)
    one = (lambda f, p: M.niqe_features_u16(f, p), lambda f, p: M.niqe_u16(f, p, nq), lambda f, p: M.brisque_features_u16(f, p),
           lambda f, p: M.brisque_u16(f, p, bq))
    two = (lambda a, b, p: M.farneback_u16(a, b, p), lambda a, b, p: M.tof_frames_u16(a, b, p), lambda a, b, p: M.tof_u16(a, b, p),
           lambda a, b, p: M.lpips_layers_u16(a, b, p, lp), lambda a, b, p: M.lpips_u16(a, b, p, lp))
    for bad in (0, 65536, -1, 1023.0, True, None):
        for call in one:
            with pytest.raises(ValueError, match="peak"):
                call(u16, bad)
        for call in two:
            with pytest.raises(ValueError, match="peak"):
                call(u16, u16, bad)
    for frames in (u16.to(torch.uint8), u16.to(torch.int16), u16.float(), u16.to(torch.float64)):      # the dtype (and no device)
        for call in one:
            with pytest.raises(ValueError):
                call(frames, 1023)
        for call in two:
            with pytest.raises(ValueError):
                call(frames, u16, 1023)
            with pytest.raises(ValueError):
                call(u16, frames, 1023)
    for call in two:                                                                                    # mismatched stacks
        with pytest.raises(ValueError):
            call(u16, u16[:1], 1023)
    with pytest.raises(ValueError):
        M.farneback_u16(u16, u16[:, :95], 1023)
    # the kernel wrappers' own keyword
    from cdfo_amd import kernels as K
    for call in (lambda p: K.niqe_mscn(u16, 96, 96, M.niqe_window(), peak=p), lambda p: K.niqe_half(u16, 96, 96, peak=p),
                 lambda p: K.brisque_mscn(u16, M.brisque_window(), peak=p), lambda p: K.brisque_half(u16, peak=p),
                 lambda p: K.tof_level(u16, u16, 96, 128, M.tof_taps(0), peak=p),
                 lambda p: K.lpips_stem(u16, torch.zeros(16, 3, 3, 3), torch.zeros(16), peak=p)):
        for bad in (0, 65536):
            with pytest.raises(ValueError, match="peak"):
                call(bad)
        with pytest.raises(ValueError):
            call(1023)                                                                                  # host tensors: refused, not run
