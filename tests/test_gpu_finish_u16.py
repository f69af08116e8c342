"""The 16-bit forms of finish.hip's kernels: cdfo_finish_frames_u16 bit for bit against its numpy statement (tests/pixfmt_ref.py), its
integer sum of squared differences against numpy int64, and ssim_u16 against the fp64 helper."""
import ctypes as C

import numpy as np
import pytest
import torch

import pixfmt_ref

pytestmark = pytest.mark.gpu
SSIM_TOL = 1e-9       # the project's device-against-oracle bound for SSIM (tests/test_gpu_finish.py, tests/test_metrics.py)
PEAKS = [1023, 4095, 65535]
# LR (H, W) -> rows of Wo = 4, 12, 8, 16, 28 samples: 8-byte stores (the narrowest row, and 12, 28), 16-byte stores (8, 16)
SIZES = [(1, 1), (2, 3), (5, 2), (3, 4), (5, 7)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _source(K, H, W, peak, seed, padded):
    """fp32 [K,4H,4W] (numpy) and the same on the device as [K,1,4H,4W], dense or a view of larger frames (pitch 4W + 8, four more
    rows, 7.0 around the frames).  Values: uniform over [-0.1, 1.1]; NaN, +-inf; for random k, float32(k) / float32(peak) and its
    two fp32 neighbours (where truncation and round-to-nearest part)."""
    rs = np.random.RandomState(seed)
    Ho, Wo = 4 * H, 4 * W
    x = rs.uniform(-0.1, 1.1, (K, Ho, Wo)).astype(np.float32)
    for k in range(K):
        n = (Ho * Wo - 4) // 3
        exact = rs.randint(0, peak + 1, min(n, 64)).astype(np.float32) / np.float32(peak)
        special = np.concatenate([np.array([np.nan, np.inf, -np.inf], np.float32), exact, np.nextafter(exact, np.float32(-1)),
                                  np.nextafter(exact, np.float32(2))])
        x[k].reshape(-1)[rs.permutation(Ho * Wo)[:special.size]] = special
    if not padded:
        return x, _dev(x[:, None])
    full = np.full((K, 1, Ho + 4, Wo + 8), 7.0, np.float32)
    full[:, 0, 2:2 + Ho, 4:4 + Wo] = x
    xd = _dev(full)[:, :, 2:2 + Ho, 4:4 + Wo]
    assert not xd.is_contiguous() or Ho == 1
    return x, xd


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("peak", PEAKS)
def test_finish_frames_u16_bit_exact(peak, H, W):
    from cdfo_amd import kernels as Kn
    for K, padded in ((1, False), (3, True), (3, False), (1, True)):
        want, xd = _source(K, H, W, peak, 100 * H + W + K, padded)
        ref = {mode: pixfmt_ref.quantise(want, mode, peak) for mode in ("trunc", "nearest")}
        assert (ref["trunc"] != ref["nearest"]).any() and ref["trunc"].max() == peak and ref["trunc"].min() == 0
        for mode in ("trunc", "nearest"):
            u16, sse = Kn.finish_frames(xd, H, W, mode=mode, peak=peak)
            assert sse is None and u16.dtype == torch.uint16 and tuple(u16.shape) == (K, 4 * H, 4 * W) and u16.is_contiguous()
            got = u16.cpu().numpy()
            assert np.array_equal(got, ref[mode]), (mode, K, padded, np.argwhere(got != ref[mode])[:5])
        dst = _dev(np.full((K, 4 * H, 4 * W), 7, np.uint16))             # a destination of the caller's; a 3-d source
        got, _ = Kn.finish_frames(xd[:, 0], H, W, dst=dst, peak=peak)
        assert got is dst and np.array_equal(dst.cpu().numpy(), ref["trunc"])


@pytest.mark.parametrize("crop", [0, 2])
@pytest.mark.parametrize("dh,dw", [(0, 0), (3, 2), (-2, -3), (2, -6), (-3, 5)])
@pytest.mark.parametrize("K,H,W,peak", [(3, 5, 7, 1023), (1, 3, 4, 65535), (2, 5, 7, 4095)])
def test_finish_frames_u16_sse_is_the_exact_integer_sum(K, H, W, peak, dh, dw, crop):
    """Ground truth of the output's size (rows of 64-bit words), wider by 2 and narrower by 6 (32-bit words; narrower: the last
    quad of a row is cut), narrower by 3 and wider by 5 (odd rows: per element); dense, inside wider frames with an odd pitch (per
    element) and, where the width allows, inside frames four samples wider (words, rows longer than the frame)."""
    from cdfo_amd import kernels as Kn
    want, xd = _source(K, H, W, peak, 20 + K + dh - dw, padded=bool(crop))
    q = pixfmt_ref.quantise(want, "trunc", peak)
    Hg, Wg = 4 * H + dh, 4 * W + dw
    rs = np.random.RandomState(20 + dh - dw + crop)
    wide = rs.randint(0, peak + 1, (K, Hg, Wg + 3 + Wg % 2)).astype(np.uint16)
    assert wide.shape[2] % 2 == 1
    cases = [(wide[:, :, :Wg].copy(), None), (wide[:, :, 3:3 + Wg], _dev(wide)[:, :, 3:3 + Wg])]
    if Wg % 2 == 0:
        wide4 = rs.randint(0, peak + 1, (K, Hg, Wg + 4)).astype(np.uint16)
        cases.append((wide4[:, :, :Wg], _dev(wide4)[:, :, :Wg]))
        cases.append((wide4[:, :, 2:2 + Wg], _dev(wide4)[:, :, 2:2 + Wg]))       # 4-byte aligned rows only
    for gt, gd in cases:
        gd = _dev(gt) if gd is None else gd
        ref = pixfmt_ref.sse(q, gt, crop)
        assert ref.min() > 0
        u16, sse = Kn.finish_frames(xd, H, W, gt=gd, crop=crop, peak=peak)
        assert sse.dtype == torch.int64 and tuple(sse.shape) == (K,)
        assert np.array_equal(sse.cpu().numpy(), ref), (sse.cpu().numpy(), ref)
        assert np.array_equal(u16.cpu().numpy(), q)


def test_finish_frames_u16_squares_beyond_31_bits():
    """All-zero output against all-65535 ground truth: every square is 4 294 836 225, which a signed 32-bit product does not hold."""
    from cdfo_amd import kernels as Kn
    x = torch.zeros((2, 1, 20, 28), device="cuda")
    for gt in (np.full((2, 20, 28), 65535, np.uint16), np.full((2, 21, 27), 65535, np.uint16)):
        u16, sse = Kn.finish_frames(x, 5, 7, gt=_dev(gt), crop=0, peak=65535)
        assert not u16.cpu().numpy().any()
        assert sse.cpu().tolist() == [20 * min(28, gt.shape[2]) * 65535 ** 2] * 2


def test_finish_frames_u16_bad_arguments():
    from cdfo_amd import _lib
    from cdfo_amd import kernels as Kn
    from cdfo_amd._lib import CdfoError
    x = torch.rand((2, 1, 32, 32), device="cuda")
    gt = _dev(np.zeros((2, 6, 32), np.uint16))
    with pytest.raises(CdfoError, match="invalid argument"):                          # crop too large for Hm = min(32, 6)
        Kn.finish_frames(x, 8, 8, gt=gt, crop=3, peak=1023)
    Kn.finish_frames(x, 8, 8, gt=gt, crop=2, peak=1023)
    flat = _dev(np.zeros(2 * 32 * 32 + 16, np.uint16))
    with pytest.raises(CdfoError, match="misaligned"):                                # destination off a 16-byte boundary
        Kn.finish_frames(x, 8, 8, dst=flat[4:4 + 2 * 32 * 32].view(2, 32, 32), peak=1023)
    with pytest.raises(CdfoError, match="misaligned"):                                # source rows off a 16-byte boundary
        Kn.finish_frames(torch.rand((2, 1, 32, 34), device="cuda")[..., 1:33], 8, 8, peak=1023)
    for bad in (dict(peak=0), dict(peak=65536), dict(peak=1023.0), dict(peak=1023, mode="floor"),
                dict(peak=1023, gt=torch.zeros((2, 6, 32), dtype=torch.uint8, device="cuda")),
                dict(peak=1023, dst=torch.zeros((2, 32, 32), dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError):
            Kn.finish_frames(x, 8, 8, **bad)
    dst = _dev(np.zeros((2, 32, 32), np.uint16))
    nb = C.c_int(0)
    lib, vp, st = _lib.lib(), Kn._vp, Kn._stream()
    tail = (0, None, 0, C.c_longlong(0), 0, 0, 0, None, 0, C.byref(nb), st)
    assert lib.cdfo_finish_frames_u16(vp(x), 32, C.c_longlong(1024), 2, 32, 32, vp(dst), 0, *tail) == -1           # peak 0
    assert lib.cdfo_finish_frames_u16(vp(x), 32, C.c_longlong(1024), 2, 32, 32, vp(dst), 65536, *tail) == -1       # peak 2^16
    assert lib.cdfo_finish_frames_u16(vp(x), 32, C.c_longlong(1024), 2, 32, 30, vp(dst), 1023, *tail) == -1        # Wo % 4
    assert lib.cdfo_finish_frames_u16(vp(x), 65536, C.c_longlong(0), 1, 65536, 65536, vp(dst), 1023, *tail) == -1
    assert lib.cdfo_finish_frames_u16(vp(x), 1 << 20, C.c_longlong(0), 1, 4096, 32, vp(dst), 1023, *tail) == -1    # rows * pitch = 2^32
    part = torch.empty(1024, dtype=torch.float64, device="cuda")
    ss = lambda *a: lib.cdfo_ssim_partials_u16(*a, vp(part), 1024, C.byref(nb), st)
    assert ss(vp(dst), 1 << 20, C.c_longlong(0), 4096, 32, vp(dst), 32, C.c_longlong(0), 32, 32, 1, 0, 1023) == -1
    assert ss(vp(dst), 32, C.c_longlong(0), 32, 32, vp(dst), 32, C.c_longlong(0), 32, 32, 1, 0, 0) == -1           # peak 0
    assert ss(vp(dst), 32, C.c_longlong(0), 32, 32, vp(dst), 32, C.c_longlong(0), 32, 32, 1, 11, 1023) == -1       # no window left
    torch.cuda.synchronize()


# --- SSIM ---------------------------------------------------------------------------------------------------------------------------
def _pair(N, shape, peak, seed):
    rs = np.random.RandomState(seed)
    a = rs.randint(0, peak + 1, (N,) + shape).astype(np.uint16)
    b = np.clip(a.astype(np.int64) + np.round(rs.randn(N, *shape) * (peak / 25.0)).astype(np.int64), 0, peak).astype(np.uint16)
    return a, b


@pytest.mark.parametrize("N,shape,crop", [(2, (19, 19), 4), (1, (11, 11), 0), (2, (27, 45), 0)])
@pytest.mark.parametrize("peak", [1023, 65535])
def test_ssim_u16_matches_the_helper(peak, N, shape, crop):
    """19x19 with crop 4 and 11x11 with crop 0 (1x1 maps), 27x45 (a 17x35 map: ragged tiles both ways); dense stacks and views of
    larger frames; a stack against itself is exactly 1."""
    from cdfo_amd import metrics as M
    a, b = _pair(N, shape, peak, shape[0] + crop)
    a[0, 0, 0], a[0, -1, -1] = peak, 0
    big = np.full((N, shape[0] + 3, shape[1] + 5), peak, np.uint16)
    big[:, 1:1 + shape[0], 2:2 + shape[1]] = b
    for bd in (_dev(b), _dev(big)[:, 1:1 + shape[0], 2:2 + shape[1]]):
        s = M.ssim_u16(_dev(a), bd, crop, peak).cpu().numpy()
        assert s.dtype == np.float64 and s.shape == (N,)
        for n in range(N):
            want = pixfmt_ref.calculate_ssim(a[n], b[n], crop, peak)
            print(f"peak {peak} {shape} crop {crop} frame {n}: SSIM {s[n]!r}, helper {want!r}, error {abs(s[n] - want):.2e}")
            assert abs(s[n] - want) < SSIM_TOL
    assert M.ssim_u16(_dev(a), _dev(a), crop, peak).cpu().tolist() == [1.0] * N


@pytest.mark.parametrize("peak", [1023, 65535])
def test_ssim_u16_of_equal_frames_is_exactly_one(peak):
    """64 random frames of 11x11 and of 19x19 with crop 4, each a 1x1 map, so a frame's SSIM is one term and nothing averages an ulp
    away: a term whose products of means are fused into the sums that follow misses 1.0 in about a sixth of such frames."""
    from cdfo_amd import metrics as M
    for shape, crop in (((11, 11), 0), ((19, 19), 4)):
        a, _ = _pair(64, shape, peak, 40 + crop)
        s = M.ssim_u16(_dev(a), _dev(a), crop, peak).cpu().numpy()
        assert s.shape == (64,) and np.array_equal(s, np.ones(64)), np.abs(s - 1.0).max()


def test_ssim_u16_over_the_common_size_and_at_peak_255():
    from cdfo_amd import metrics as M
    a, _ = _pair(2, (27, 45), 1023, 1)
    g, _ = _pair(2, (30, 41), 1023, 2)
    s = M.ssim_u16(_dev(a), _dev(g), 2, 1023).cpu().numpy()
    for n in range(2):
        assert abs(s[n] - pixfmt_ref.calculate_ssim(a[n, :27, :41], g[n, :27, :41], 2, 1023)) < SSIM_TOL
    rs = np.random.RandomState(3)
    a8 = rs.randint(0, 256, (2, 27, 45)).astype(np.uint8)
    b8 = np.clip(a8.astype(int) + np.round(rs.randn(2, 27, 45) * 10).astype(int), 0, 255).astype(np.uint8)
    s8 = M.ssim_u8(_dev(a8), _dev(b8), 4).cpu().numpy()
    s16 = M.ssim_u16(_dev(a8.astype(np.uint16)), _dev(b8.astype(np.uint16)), 4, 255).cpu().numpy()
    assert np.abs(s8 - s16).max() <= 1e-12
    with pytest.raises(ValueError):
        M.ssim_u16(_dev(a8), _dev(b8), 4, 255)                             # 8-bit stacks
    with pytest.raises(ValueError):
        M.ssim_u16(_dev(a), _dev(a), 4, 0)
