"""The device kernels of sequence evaluation (finish.hip): cdfo_finish_frames bit for bit against its numpy statement, its integer
sum of squared differences against numpy int64, and the 8-bit PSNR / SSIM wrappers against oracle/metrics_ref.py."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SSIM_TOL = 1e-9       # the bound tests/test_metrics.py holds the fp32-input SSIM kernel to


def _numpy_quantise(x, mode):
    """clip to [0,1] (NaN -> 0), one fp32 multiply by 255, truncation / round-half-even: written out here, not imported."""
    v = np.where(np.isnan(x), np.float32(0), x.astype(np.float32))
    v = np.clip(v, np.float32(0), np.float32(1)) * np.float32(255.0)
    assert v.dtype == np.float32
    return (np.rint(v) if mode == "nearest" else v).astype(np.uint8)


def _source(K, H, W, seed, pitched=False):
    """[K,1,4Hp,4Wp] fp32 with Hp, Wp the multiples of 8 above H, W: values over [-0.2, 1.2], every k/255, +-0, +-inf, NaN inside
    the cropped region, and NaN in the padding (which must not be read into the result).  pitched: a view with a row pitch and a
    frame stride larger than the frame."""
    Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    g = torch.Generator().manual_seed(seed)
    full = torch.rand((K, 1, 4 * Hp + 4, 4 * Wp + 8), generator=g) * 1.4 - 0.2
    x = full[:, :, 2:2 + 4 * Hp, 4:4 + 4 * Wp] if pitched else full[:, :, :4 * Hp, :4 * Wp].contiguous()
    special = torch.cat([torch.arange(256, dtype=torch.float64).div(255.0).float(), torch.arange(256).float() / 255.0,
                         torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1.0, 0.5 / 255, 1.5 / 255, 2.5 / 255])])
    for k in range(K):
        for r, row in enumerate(special.split(4 * W)):            # every special value inside the cropped region of every frame
            x[k, 0, r + k, :row.numel()] = row
        x[k, 0, 4 * H - 1, 4 * W - 9:4 * W] = special[-9:]         # and at the last pixels of the last row
    if 4 * Hp > 4 * H:
        x[:, :, 4 * H:, :] = float("nan")
    if 4 * Wp > 4 * W:
        x[:, :, :, 4 * W:] = float("nan")
    dev = full.cuda()
    xd = dev[:, :, 2:2 + 4 * Hp, 4:4 + 4 * Wp] if pitched else x.cuda()
    if pitched:
        xd.copy_(x)
        assert not xd.is_contiguous() and xd.stride(2) == 4 * Wp + 8
    return x.numpy()[:, 0, :4 * H, :4 * W], xd


@pytest.mark.parametrize("mode", ["trunc", "nearest"])
@pytest.mark.parametrize("K,H,W,pitched", [(1, 21, 27, False), (3, 21, 27, True), (3, 16, 24, False), (1, 16, 24, True),
                                           (2, 9, 10, False)])
def test_finish_frames_bit_exact(K, H, W, pitched, mode):
    """21x27 in 24x32 -> 84x108 of 96x128 (108 = 4 * 27: 4-byte stores), 16x24 -> 64x96 (16-byte stores), 9x10 -> 36x40 (8-byte
    stores); K = 1, 2, 3; dense sources and a view whose pitch and frame stride exceed the frame."""
    from cdfo_amd import kernels as Kn
    want, xd = _source(K, H, W, 10 * K + H, pitched)
    u8, sse = Kn.finish_frames(xd, H, W, mode=mode)
    assert sse is None and u8.dtype == torch.uint8 and tuple(u8.shape) == (K, 4 * H, 4 * W) and u8.is_contiguous()
    ref = torch.from_numpy(_numpy_quantise(want, mode))
    assert torch.equal(u8.cpu(), ref)
    if mode == "trunc":            # the reference's writer itself, where it is defined (no NaN)
        fin = ~np.isnan(want)
        assert np.array_equal(u8.cpu().numpy()[fin], (np.clip(np.where(fin, want, np.float32(0)), 0, 1) * 255.0).astype(np.uint8)[fin])
    # a destination of the caller's, filled in place; 3-d sources are taken too
    dst = torch.full((K, 4 * H, 4 * W), 7, dtype=torch.uint8, device="cuda")
    got, _ = Kn.finish_frames(xd[:, 0], H, W, mode=mode, dst=dst)
    assert got is dst and torch.equal(dst.cpu(), ref)


@pytest.mark.parametrize("crop", [0, 4])
@pytest.mark.parametrize("dh,dw", [(0, 0), (2, 0), (0, -4), (2, -4)])
@pytest.mark.parametrize("K,H,W", [(3, 21, 27), (1, 16, 24)])
def test_finish_frames_sse_is_the_exact_integer_sum(K, H, W, dh, dw, crop):
    """Ground truth of the output's size, 2 rows taller, 4 columns narrower, and both; a dense stack and a view of wider frames (byte
    loads instead of words)."""
    from cdfo_amd import kernels as Kn
    want, xd = _source(K, H, W, 77 + K)
    Ho, Wo, Hg, Wg = 4 * H, 4 * W, 4 * H + dh, 4 * W + dw
    rs = np.random.RandomState(5 + dh - dw + crop)
    gt = rs.randint(0, 256, (K, Hg, Wg + 3)).astype(np.uint8)
    q = _numpy_quantise(want, "trunc").astype(np.int64)
    Hm, Wm = min(Ho, Hg), min(Wo, Wg)
    for view in (gt[:, :, :Wg].copy(), gt[:, :, 3:]):
        ref = ((q[:, crop:Hm - crop, crop:Wm - crop] - view[:, crop:Hm - crop, crop:Wm - crop].astype(np.int64)) ** 2).sum(axis=(1, 2))
        gd = torch.from_numpy(gt).cuda()[:, :, 3:] if not view.flags["C_CONTIGUOUS"] else torch.from_numpy(view).cuda()
        u8, sse = Kn.finish_frames(xd, H, W, gt=gd, crop=crop)
        assert sse.dtype == torch.int64 and tuple(sse.shape) == (K,)
        assert np.array_equal(sse.cpu().numpy(), ref), (sse.cpu().numpy(), ref)
        assert torch.equal(u8.cpu(), torch.from_numpy(q.astype(np.uint8)))


# --- PSNR / SSIM of 8-bit frames --------------------------------------------------------------------------------------------------
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2        # metric/psnr_ssim.py:329-330


def _hand_cases():
    """The closed-form SSIM cases of tests/test_metrics.py, restated (8-bit valued): constant frames c1, c2 give
    (2 c1 c2 + C1) / (c1^2 + c2^2 + C1); a vertical step edge a = 255 [x >= e] against b = alpha a with 255 alpha an integer, where a
    window whose Gaussian weight right of the edge is phi has mu1 = 255 phi, sigma1^2 = 255^2 phi (1 - phi), mu2 = alpha mu1,
    sigma2^2 = alpha^2 sigma1^2, sigma12 = alpha sigma1^2, averaged over the valid columns."""
    cases = [(np.full((30, 34), 100), np.full((30, 34), 120), 0, 0.9836109249983688),          # (24000 + C1) / (24400 + C1)
             (np.full((30, 34), 100), np.full((30, 34), 120), 4, 0.9836109249983688),
             (np.zeros((24, 28)), np.full((24, 28), 255), 0, 9.999000099990003e-05)]            # C1 / (255^2 + C1)
    taps = [np.exp(-((k - 5.0) ** 2) / 4.5) for k in range(11)]
    taps = [t / sum(taps) for t in taps]
    for (H, W, e, level, crop) in ((24, 40, 20, 51, 0), (32, 48, 25, 204, 4)):                 # alpha = 0.2, 0.8
        alpha = level / 255.0
        a = np.zeros((H, W))
        a[:, e:] = 255
        b = np.zeros((H, W))
        b[:, e:] = level
        vals = []
        for x in range(crop, W - crop - 10):
            phi = sum(taps[k] for k in range(11) if x + k >= e)
            mu2, s = (255.0 * phi) ** 2, 255.0 ** 2 * phi * (1.0 - phi)
            vals.append((2 * alpha * mu2 + C1) * (2 * alpha * s + C2) / (((1 + alpha * alpha) * mu2 + C1) * ((1 + alpha * alpha) * s + C2)))
        cases.append((a, b, crop, float(np.mean(vals))))
    return [(a.astype(np.uint8), b.astype(np.uint8), crop, want) for a, b, crop, want in cases]


def test_ssim_u8_hand_derived_vectors():
    from cdfo_amd import metrics as M
    from oracle.metrics_ref import calculate_ssim
    for a, b, crop, want in _hand_cases():
        assert abs(calculate_ssim(a, b, crop) - want) < 1e-12                      # the restated cases are the oracle's own
        got = M.ssim_u8(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), crop).item()
        print(f"hand case {a.shape} crop {crop}: device {got!r}, closed form {want!r}")
        assert abs(got - want) < SSIM_TOL, (a.shape, crop, got, want)


def _pair(N, shape, seed):
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 256, (N,) + shape).astype(np.uint8)
    b = np.clip(a.astype(int) + np.round(rs.randn(N, *shape) * 10).astype(int), 0, 255).astype(np.uint8)
    return a, b


@pytest.mark.parametrize("N,shape,crop", [(3, (84, 108), 4), (3, (84, 108), 0), (1, (64, 96), 4), (1, (40, 300), 4), (2, (19, 19), 4),
                                          (1, (70, 45), 0)])
def test_psnr_and_ssim_u8_match_the_oracle(N, shape, crop):
    """Random pairs at the sizes above, 40x300 (a row of the map spans ten tiles), 19x19 with crop 4 (a 1x1 map), 70x45 (several tile
    rows, ragged both ways): PSNR equal to the oracle's with ==, SSIM within 1e-9."""
    from cdfo_amd import metrics as M
    from oracle.metrics_ref import calculate_psnr, calculate_ssim
    a, b = _pair(N, shape, shape[0] + crop)
    b[0, crop:crop + 3] = a[0, crop:crop + 3]
    ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    p, s = M.psnr_u8(ad, bd, crop), M.ssim_u8(ad, bd, crop).cpu().numpy()
    assert p.dtype == np.float64 and p.shape == (N,) and s.dtype == np.float64
    for n in range(N):
        want_p, want_s = calculate_psnr(a[n], b[n], crop), calculate_ssim(a[n], b[n], crop)
        print(f"{shape} crop {crop} frame {n}: PSNR {p[n]!r} (oracle {want_p!r}), SSIM error {abs(s[n] - want_s):.2e}")
        assert p[n] == want_p
        assert abs(s[n] - want_s) < SSIM_TOL
    # identical frames
    assert np.all(np.isinf(M.psnr_u8(ad, ad, crop))) and np.all(M.psnr_u8(ad, ad, crop) > 0)
    assert (M.ssim_u8(ad, ad, crop).cpu() - 1.0).abs().max().item() < SSIM_TOL


def test_u8_metrics_compare_over_the_common_size():
    """Stacks of different sizes and pitches: the result 84x108 against ground truth 86x108 and 84x104 held inside larger frames."""
    from cdfo_amd import metrics as M
    from oracle.metrics_ref import calculate_psnr, calculate_ssim
    a, _ = _pair(2, (84, 108), 1)
    big, _ = _pair(2, (90, 120), 2)
    for (h, w) in ((86, 108), (84, 104), (86, 104)):
        view = torch.from_numpy(big).cuda()[:, 1:1 + h, 5:5 + w]
        g = big[:, 1:1 + h, 5:5 + w]
        hm, wm = min(84, h), min(108, w)
        p, s = M.psnr_u8(torch.from_numpy(a).cuda(), view, 4), M.ssim_u8(torch.from_numpy(a).cuda(), view, 4).cpu().numpy()
        for n in range(2):
            assert p[n] == calculate_psnr(a[n, :hm, :wm], g[n, :hm, :wm], 4)
            assert abs(s[n] - calculate_ssim(a[n, :hm, :wm], g[n, :hm, :wm], 4)) < SSIM_TOL
        s2, n2 = M.sse_u8(view, torch.from_numpy(a).cuda(), 4)
        assert n2 == (hm - 8) * (wm - 8) and s2.dtype == torch.int64


def test_bad_arguments_raise():
    from cdfo_amd import _lib
    from cdfo_amd import kernels as Kn
    from cdfo_amd import metrics as M
    from cdfo_amd._lib import CdfoError
    x = torch.rand((2, 1, 32, 32), device="cuda")
    gt = torch.zeros((2, 6, 32), dtype=torch.uint8, device="cuda")
    with pytest.raises(CdfoError, match="invalid argument"):                          # crop too large for Hm = min(32, 6)
        Kn.finish_frames(x, 8, 8, gt=gt, crop=3)
    Kn.finish_frames(x, 8, 8, gt=gt, crop=2)
    with pytest.raises(CdfoError, match="invalid argument"):                          # no 11x11 window left
        M.ssim_u8(gt, gt, 0)
    flat = torch.empty(2 * 32 * 32 + 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(CdfoError, match="misaligned"):                                # destination off a 16-byte boundary
        Kn.finish_frames(x, 8, 8, dst=flat[4:4 + 2 * 32 * 32].view(2, 32, 32))
    with pytest.raises(CdfoError, match="misaligned"):                                # source rows off a 16-byte boundary
        Kn.finish_frames(torch.rand((2, 1, 32, 34), device="cuda")[..., 1:33], 8, 8)
    with pytest.raises(ValueError):
        Kn.finish_frames(x, 8, 8, mode="floor")
    with pytest.raises(ValueError):
        Kn.finish_frames(x, 9, 8)                                                     # 36 rows asked of a 32-row tensor
    # a frame beyond the 32-bit offsets: refused from the arguments alone, before anything is launched (the pointers are those
    # of the small tensors above)
    dst = torch.empty((2, 32, 32), dtype=torch.uint8, device="cuda")
    nb = C.c_int(0)
    lib, vp, st = _lib.lib(), Kn._vp, Kn._stream()
    assert lib.cdfo_finish_frames(vp(x), 65536, C.c_longlong(0), 1, 65536, 65536, vp(dst), 0, None, 0, C.c_longlong(0), 0, 0, 0, None, 0,
                                  C.byref(nb), st) == -1
    assert lib.cdfo_finish_frames(vp(x), 1 << 20, C.c_longlong(0), 1, 4096, 32, vp(dst), 0, None, 0, C.c_longlong(0), 0, 0, 0, None, 0,
                                  C.byref(nb), st) == -1                              # rows * pitch = 2^32
    part = torch.empty(1024, dtype=torch.float64, device="cuda")
    assert lib.cdfo_metric_partials_u8(vp(dst), 1 << 20, C.c_longlong(0), 4096, 32, vp(dst), 32, C.c_longlong(0), 32, 32, 1, 0, 0,
                                       vp(part), 1024, C.byref(nb), st) == -1
    torch.cuda.synchronize()
