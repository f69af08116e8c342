"""MS-SSIM without a GPU: the numpy oracle against closed forms and the SSIM oracle, the host-side combine, the result tuples and their
log lines, the evaluator's size check and the C ABI's argument validation."""
import ctypes as C
import os

import numpy as np
import pytest

import msssim_ref as ref


@pytest.mark.parametrize("peak,p,q", [(255, 100, 110), (255, 0, 255), (1023, 512, 500), (65535, 40000, 65535)])
def test_ref_matches_the_closed_form_on_constant_frames(peak, p, q):
    """a == p, b == q everywhere: the variances vanish, every cs is 1, every l is l(p, q), MS-SSIM = l(p, q)^w[4]."""
    a, b = np.full((190, 180), p, np.uint16), np.full((190, 180), q, np.uint16)
    C1 = (0.01 * peak) ** 2
    lum = (2.0 * p * q + C1) / (float(p) ** 2 + float(q) ** 2 + C1)
    c = ref.components(a, b, 2, peak)
    assert np.abs(c[:, 0] - 1.0).max() < 1e-12 and np.abs(c[:, 1] - lum).max() < 1e-12
    assert abs(ref.combine(c) - lum ** 0.1333) < 1e-12


def test_ref_level_sizes_and_level_0_is_the_ssim_oracle():
    from oracle.metrics_ref import calculate_ssim
    a, b = ref.correlated_pair(1, (183, 205), 255, 20)
    assert ref.components(a[0], b[0], 0, 255)[0, 1] == pytest.approx(calculate_ssim(a[0], b[0], 0), abs=1e-15)
    assert ref.components(a[0], b[0], 3, 255)[0, 1] == pytest.approx(calculate_ssim(a[0], b[0], 3), abs=1e-15)
    x = np.arange(7 * 5, dtype=np.float64).reshape(7, 5)
    assert ref.pool2(x).shape == (3, 2) and ref.pool2(x)[0, 0] == (0 + 1 + 5 + 6) / 4.0 and ref.pool2(x)[2, 1] == (22 + 23 + 27 + 28) / 4.0
    with pytest.raises(ValueError):
        ref.components(a[0], b[0], 4, 255)               # 175 rows


def test_combine_matches_the_ref_and_clamps_at_zero():
    import torch
    from cdfo_amd import metrics as M
    assert M.msssim_min_size == 176 == ref.MIN_SIZE
    rs = np.random.RandomState(3)
    c = rs.uniform(0.05, 1.0, (6, 5, 2))
    c[2, 1, 0] = -0.25                                   # a negative M_cs: the product is 0
    c[3, 2, 1] = -0.5                                    # a negative M_ssim at a level whose M_ssim is not used
    want = np.array([ref.combine(x) for x in c])
    for got in (M.msssim_from_components(c), M.msssim_from_components(torch.from_numpy(c))):
        assert got.dtype == np.float64 and got.shape == (6,)
        assert np.abs(got - want).max() < 1e-15
        assert got[2] == 0.0 and got[3] > 0.0
    assert M.msssim_from_components(np.zeros((0, 5, 2))).shape == (0,)
    assert abs(float(M.msssim_from_components(c[0])) - want[0]) < 1e-15
    with pytest.raises(ValueError):
        M.msssim_from_components(np.zeros((5, 3)))


def test_result_tuples_keep_their_arity_and_log_lines():
    from cdfo_amd import evaluate as E
    z = np.zeros(0)
    r = E.SequenceResult(np.array([30.0]), np.array([0.9]), 30.0, 0.9, 1, 0.5, 1.0)
    assert len(r.msssim) == 0 and np.isnan(r.mean_msssim)
    assert E.format_log(r, "seq") == "seq Average PSNR/SSIM: 30.000/0.90000"
    r = r._replace(msssim=np.array([0.987654321]), mean_msssim=0.987654321)
    assert E.format_log(r, "seq") == "seq Average PSNR/SSIM: 30.000/0.90000 MS-SSIM: 0.98765"
    y = E.YuvResult(z, z, z, z, z, 31.0, 40.0, 41.0, 0.8, 33.375, 2, 0.5, 1.0)
    assert len(y.msssim) == 0 and np.isnan(y.mean_msssim)
    assert E.format_log_yuv(y, "q") == "q Average PSNR/SSIM: 31.000/0.80000 PSNR-U/V/YUV: 40.000/41.000/33.375"
    y = y._replace(msssim=np.array([0.5, 0.75]), mean_msssim=0.625)
    assert E.format_log_yuv(y, "q") == "q Average PSNR/SSIM: 31.000/0.80000 PSNR-U/V/YUV: 40.000/41.000/33.375 MS-SSIM: 0.62500"


def test_evaluators_refuse_a_region_below_the_minimum_before_the_model(tmp_path):
    """40x40 LR frames: a 160x160 result, 152x152 inside the border.  model=None: nothing may touch it before the check."""
    from cdfo_amd import evaluate as E
    lr, side, gt = E.write_synthetic_sequence(str(tmp_path / "png"), 2, 40, 40, seed=1)
    with pytest.raises(ValueError, match="176.*152 x 152"):
        E.evaluate_sequence(None, lr, side, gt_dir=gt, save_dir=str(tmp_path / "out"), msssim=True)
    lr_yuv, side, gt_yuv = E.write_synthetic_sequence_yuv(str(tmp_path / "yuv"), 2, 40, 40, seed=1)
    with pytest.raises(ValueError, match="176.*152 x 152"):
        E.evaluate_yuv(None, lr_yuv, 40, 40, side, gt_yuv=gt_yuv, save_yuv=str(tmp_path / "out.yuv"), msssim=True)
    assert not os.path.exists(str(tmp_path / "out")) and not os.path.exists(str(tmp_path / "out.yuv"))      # nor was anything made


def test_abi_argument_validation_needs_no_gpu():
    """Everything is refused from the arguments alone, before any launch: the pointers are never dereferenced."""
    from cdfo_amd import _lib
    lib = _lib.lib()
    nb = (C.c_int * 5)()
    p = C.c_void_p(1 << 20)                              # any aligned non-null address
    ll = C.c_longlong
    big = ll(1 << 40)

    def u8(a=p, b=p, H=184, W=200, crop=4, pyr=p, pyr_bytes=big, part=p, cap=10240, N=1):
        return lib.cdfo_msssim_partials_u8(a, W, ll(H * W), H, W, b, W, ll(H * W), H, W, N, crop, pyr, pyr_bytes, part, cap, nb, None)

    def u16(peak=1023, W=200, part=p, pyr=p, a=p):
        return lib.cdfo_msssim_partials_u16(a, W, ll(184 * W), 184, W, p, W, ll(184 * W), 184, W, 1, 4, peak, pyr, big, part, 10240, nb, None)

    for bad in (u8(a=None), u8(b=None), u8(pyr=None), u8(part=None), u16(a=None)):
        assert bad == -1
    assert u8(H=183) == -1 and u8(W=183) == -1 and u8(H=175, crop=0) == -1 and u16(W=183) == -1     # 175 inside the border
    assert u8(crop=-1) == -1 and u8(N=0) == -1 and u16(peak=0) == -1 and u16(peak=65536) == -1
    # 184x200, crop 4: 176x192, tiles of 16x32 outputs: 11x6 + 5x3 + 3x2 + 1 + 1 = 89 blocks, 178 doubles per frame
    assert u8(cap=177) == -1 and u8(N=3, cap=533) == -1
    need = lib.cdfo_msssim_pyramid_bytes(176, 192, 1)
    assert need == 2 * 4 * (88 * 96 + 44 * 48 + 22 * 24 + 11 * 12)
    assert lib.cdfo_msssim_pyramid_bytes(176, 192, 3) == 3 * need and lib.cdfo_msssim_pyramid_bytes(175, 192, 1) == 0
    assert u8(pyr_bytes=ll(need - 1)) == -1
    assert u8(H=1 << 20, W=1 << 12) == -1                # rows * pitch beyond the 32-bit offsets
    assert u8(part=C.c_void_p((1 << 20) + 4)) == -2 and u8(pyr=C.c_void_p((1 << 20) + 2)) == -2     # CDFO_EALIGN
    assert u16(part=C.c_void_p((1 << 20) + 4)) == -2 and u16(a=C.c_void_p((1 << 20) + 1)) == -2
