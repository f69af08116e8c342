"""cdfo_amd.metrics.msssim_u8 / msssim_u16 on the GPU against the numpy statement of the definition (tests/msssim_ref.py).

The pairs are CORRELATED (b = a + noise): for independent frames every M_cs is near 0 and the powers of the combine amplify rounding
without bound.  Every oracle component is asserted to be at least 0.1 before anything is compared with it."""
import numpy as np
import pytest
import torch

import msssim_ref as ref

pytestmark = pytest.mark.gpu
SSIM_TOL = 1e-9       # the project's device-against-oracle SSIM bound (tests/test_gpu_finish.py), here for each of the ten means

CASES = [(255, (184, 200), 4, 20),        # level 4 is 11x12: a 1x2 map
         (255, (176, 176), 0, 20),        # the minimum: a 1x1 map at level 4
         (255, (191, 213), 4, 40),        # 183x205: odd at levels 0, 1 and 2, a row or column dropped each time
         (255, (360, 200), 4, 20),        # several tile rows, a ragged tile edge at every level
         (1023, (185, 230), 4, 120),      # 10-bit constants
         (65535, (176, 240), 0, 6000)]    # squares above 2^31, pyramid sums up to 2^24


def _device(peak, a, b, crop, **kw):
    from cdfo_amd import metrics as M
    if peak == 255:
        return M.msssim_u8(a, b, crop, **kw)
    return M.msssim_u16(a, b, crop, peak, **kw)


@pytest.mark.parametrize("peak,shape,crop,sigma", CASES)
def test_components_and_value_match_the_oracle(peak, shape, crop, sigma):
    """N = 3, frame 1 of b equal to a's: the ten means within SSIM_TOL, the combined value within its first-order propagation,
    level 0's M_ssim within it of ssim_u8 / ssim_u16, and the identical frame at 1 (exactly 1 in the 16-bit form)."""
    from cdfo_amd import metrics as M
    a, b = ref.correlated_pair(3, shape, peak, sigma, seed=1)
    ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    x, c = _device(peak, ad, bd, crop, components=True)
    assert x.dtype == torch.float64 and x.shape == (3,) and c.dtype == torch.float64 and c.shape == (3, 5, 2)
    assert torch.equal(x, _device(peak, ad, bd, crop))
    x, c = x.cpu().numpy(), c.cpu().numpy()
    ssim = (M.ssim_u8(ad, bd, crop) if peak == 255 else M.ssim_u16(ad, bd, crop, peak)).cpu().numpy()
    for n in range(3):
        want = ref.components(a[n], b[n], crop, peak)
        assert want.min() >= 0.1, want
        bound = ref.propagated_bound(want, SSIM_TOL)
        print(f"peak {peak} {shape} crop {crop} frame {n}: smallest component {want.min():.4f}, worst mean error "
              f"{np.abs(c[n] - want).max():.2e}, value {x[n]!r} error {abs(x[n] - ref.combine(want)):.2e} (bound {bound:.2e}), "
              f"|M_ssim[0] - ssim| {abs(c[n, 0, 1] - ssim[n]):.2e}")
        assert np.abs(c[n] - want).max() < SSIM_TOL
        assert abs(x[n] - ref.combine(want)) < bound
        assert abs(c[n, 0, 1] - ssim[n]) < SSIM_TOL
    assert abs(1.0 - x[1]) < SSIM_TOL
    if peak != 255:
        assert x[1] == 1.0 and np.all(c[1] == 1.0)


def test_compares_over_the_common_size():
    """Stacks of different sizes and pitches: 184x200 against 186x200, 184x196 and 186x196 held inside larger frames."""
    from cdfo_amd import metrics as M
    a, noisy = ref.correlated_pair(2, (184, 200), 255, 20, seed=2)
    big = np.random.RandomState(5).randint(0, 256, (2, 192, 212)).astype(np.uint8)
    big[:, 1:185, 5:205] = noisy
    ad = torch.from_numpy(a).cuda()
    for (h, w) in ((186, 200), (184, 196), (186, 196)):
        view, g = torch.from_numpy(big).cuda()[:, 1:1 + h, 5:5 + w], big[:, 1:1 + h, 5:5 + w]
        x, c = M.msssim_u8(ad, view, 4, components=True)
        x2 = M.msssim_u8(view, ad, 4)                                         # the pitched stack in the first place
        for n in range(2):
            want = ref.components(a[n], g[n], 4, 255)
            assert want.min() >= 0.1
            assert np.abs(c[n].cpu().numpy() - want).max() < SSIM_TOL
            assert abs(x[n].item() - ref.combine(want)) < ref.propagated_bound(want, SSIM_TOL)
            assert abs(x2[n].item() - ref.combine(want)) < ref.propagated_bound(want, SSIM_TOL)


def test_sixteen_frames_are_two_stacks_of_eight():
    """The grid runs over the frames: one call on 16 gives what two calls on 8 give, bit for bit; a shared scratch sized for more
    frames than a call has changes nothing."""
    from cdfo_amd import metrics as M
    a, b = ref.correlated_pair(16, (184, 200), 255, 20, seed=3)
    ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    whole = M.msssim_components(ad, bd, 4)
    halves = torch.cat([M.msssim_components(ad[:8], bd[:8], 4), M.msssim_components(ad[8:], bd[8:], 4)])
    assert whole.shape == (16, 5, 2) and torch.equal(whole, halves)
    scratch = M.msssim_scratch(16, 176, 192, ad.device)
    assert torch.equal(M.msssim_components(ad[3:8], bd[3:8], 4, scratch=scratch), whole[3:8])
    want = ref.components(a[15], b[15], 4, 255)
    assert np.abs(whole[15].cpu().numpy() - want).max() < SSIM_TOL


def test_bad_arguments_raise():
    from cdfo_amd import metrics as M
    from cdfo_amd._lib import CdfoError
    z8 = torch.zeros((1, 183, 200), dtype=torch.uint8, device="cuda")
    z16 = torch.from_numpy(np.zeros((1, 183, 200), np.uint16)).cuda()
    with pytest.raises(CdfoError, match="invalid argument"):                  # 175 rows inside the border
        M.msssim_u8(z8, z8, 4)
    with pytest.raises(CdfoError, match="invalid argument"):
        M.msssim_u16(z16[:, :175], z16[:, :175], 0, 1023)
    M.msssim_u8(z8, z8, 3)                                                    # 177 rows
    with pytest.raises(ValueError):
        M.msssim_u8(z8.cpu(), z8.cpu(), 3)                                    # device tensors only
    with pytest.raises(ValueError):
        M.msssim_u16(z8, z8, 3, 1023)                                         # uint16 samples expected
    with pytest.raises(ValueError):
        M.msssim_u16(z16, z16, 3, 65536)
    with pytest.raises(ValueError):
        M.msssim_u8(z8, torch.cat([z8, z8]), 3)
    for wrong in (M.msssim_scratch(1, 176, 200, z8.device), torch.empty(1 << 20, device="cuda"), M.msssim_scratch(1, 177, 194, "cpu")):
        with pytest.raises(ValueError, match="scratch"):                      # another region, not a scratch, another device
            M.msssim_components(z8, z8, 3, scratch=wrong)
    with pytest.raises(ValueError, match="scratch"):                          # too few frames
        M.msssim_components(torch.cat([z8, z8]), torch.cat([z8, z8]), 3, scratch=M.msssim_scratch(1, 177, 194, z8.device))
