"""cdfo_chroma_up4_u16 (chroma.hip): the x4 chroma filter on 16-bit samples bit for bit against its numpy statement clipped to the peak
(tests/pixfmt_ref.py over tests/chroma_ref.py's integer sums), and its integer sum of squared differences against numpy int64.  The
shapes and the size / crop grid are tests/test_gpu_chroma.py's."""
import ctypes as C

import numpy as np
import pytest
import torch

from chroma_ref import up4_sums
from pixfmt_ref import contents, sse as _sse, up4

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 3), (5, 7), (17, 33), (9, 17)]
PEAKS = [1023, 65535]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_planes(p, pitched, peak):
    """p uint16 [N,h,w] -> the same planes on the device: a dense stack, or a view whose pitch and plane stride exceed the plane, with
    the peak everywhere outside the planes (which must never be read into the result)."""
    if not pitched:
        return _dev(p)
    N, h, w = p.shape
    full = np.full((N, h + 3, w + 5), peak, np.uint16)
    full[:, 1:1 + h, 2:2 + w] = p
    view = _dev(full)[:, 1:1 + h, 2:2 + w]
    assert view.stride(1) == w + 5 and view.stride(0) == (h + 3) * (w + 5)
    return view


@pytest.mark.parametrize("N,pitched", [(1, False), (2, True), (6, False), (6, True)])
@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("peak", PEAKS)
def test_chroma_up4_u16_bit_exact(peak, h, w, N, pitched):
    from cdfo_amd import kernels as Kn
    for name, p in contents((N, h, w), 1000 * h + 10 * w + N, peak).items():
        want = up4(p, peak)
        assert want.dtype == np.uint16
        if name != "random" and min(h, w) >= 5:          # the sums leave [0, peak] on both sides: both clamps are in the expectation
            s = (up4_sums(p) + 8192) >> 14
            assert s.min() < 0 and s.max() > peak and want.min() == 0 and want.max() == peak
        out, sse = Kn.chroma_up4(_device_planes(p, pitched, peak), peak=peak)
        assert sse is None and out.dtype == torch.uint16 and tuple(out.shape) == (N, 4 * h, 4 * w) and out.is_contiguous()
        got = out.cpu().numpy()
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])
    dst = _dev(np.full((N, 4 * h, 4 * w), 7, np.uint16))                 # a destination of the caller's; a single plane [h,w]
    got, _ = Kn.chroma_up4(_device_planes(p, pitched, peak), dst=dst, peak=peak)
    assert got is dst and np.array_equal(dst.cpu().numpy(), want)
    one, _ = Kn.chroma_up4(_device_planes(p, pitched, peak)[0], peak=peak)
    assert tuple(one.shape) == (1, 4 * h, 4 * w) and np.array_equal(one.cpu().numpy()[0], want[0])


@pytest.mark.parametrize("crop", [0, 2])
@pytest.mark.parametrize("dh,dw", [(0, 0), (2, 3), (-2, -4), (2, -4), (-3, 1)])
@pytest.mark.parametrize("N,h,w,peak", [(2, 5, 7, 65535), (3, 17, 33, 1023)])
def test_chroma_up4_u16_sse_is_the_exact_integer_sum(N, h, w, peak, dh, dw, crop):
    """Ground truth of the output's size, larger, smaller and one of each; a dense stack (64-bit words where its rows allow, else
    32-bit words or single samples), a view of wider frames with an odd pitch (single samples), and views of frames four samples
    wider at an 8- and a 4-byte offset (words, rows longer than the frame); the source dense and pitched."""
    from cdfo_amd import kernels as Kn
    p = contents((N, h, w), 31 * h + dh - dw + crop, peak)["random"]
    want = up4(p, peak)
    Hg, Wg = 4 * h + dh, 4 * w + dw
    rs = np.random.RandomState(5 + h + dh - dw + crop)
    wide = rs.randint(0, peak + 1, (N, Hg, Wg + 3 + Wg % 2)).astype(np.uint16)
    assert wide.shape[2] % 2 == 1                                            # an odd pitch
    cases = [(np.ascontiguousarray(wide[:, :, :Wg]), None), (wide[:, :, 3:3 + Wg], _dev(wide)[:, :, 3:3 + Wg])]
    if Wg % 2 == 0:
        wide4 = rs.randint(0, peak + 1, (N, Hg, Wg + 4)).astype(np.uint16)
        cases.append((wide4[:, :, :Wg], _dev(wide4)[:, :, :Wg]))
        cases.append((wide4[:, :, 2:2 + Wg], _dev(wide4)[:, :, 2:2 + Wg]))
    for gt, gd in cases:
        gd = _dev(gt) if gd is None else gd
        ref = _sse(want, gt, crop)
        assert ref.min() > 0
        for pitched in (False, True):
            out, sse = Kn.chroma_up4(_device_planes(p, pitched, peak), gt=gd, crop=crop, peak=peak)
            assert sse.dtype == torch.int64 and tuple(sse.shape) == (N,)
            assert np.array_equal(sse.cpu().numpy(), ref), (sse.cpu().numpy(), ref)
            assert np.array_equal(out.cpu().numpy(), want)


def test_chroma_up4_u16_wide_squares_and_bad_arguments():
    from cdfo_amd import _lib
    from cdfo_amd import kernels as Kn
    from cdfo_amd._lib import CdfoError
    q = contents((2, 9, 17), 3, 65535)["binary"]
    worst = np.where(up4(q, 65535) >= 32768, 0, 65535).astype(np.uint16)     # squares up to 65535^2, beyond 31 bits
    assert (up4(q, 65535) == 0).any() and (up4(q, 65535) == 65535).any()
    out, sse = Kn.chroma_up4(_dev(q), gt=_dev(worst), crop=0, peak=65535)
    assert np.array_equal(sse.cpu().numpy(), _sse(up4(q, 65535), worst, 0))
    out, sse = Kn.chroma_up4(_dev(q), gt=_dev(up4(q, 65535)), crop=0, peak=65535)
    assert sse.cpu().tolist() == [0, 0]
    src = _dev(np.zeros((2, 5, 7), np.uint16))
    gt = _dev(np.zeros((2, 6, 28), np.uint16))
    with pytest.raises(CdfoError, match="invalid argument"):                          # crop leaves nothing of Hm = min(20, 6)
        Kn.chroma_up4(src, gt=gt, crop=3, peak=1023)
    Kn.chroma_up4(src, gt=gt, crop=2, peak=1023)
    for bad in (dict(), dict(peak=0), dict(peak=65536), dict(peak=1023, gt=torch.zeros((2, 6, 28), dtype=torch.uint8, device="cuda")),
                dict(peak=1023, dst=torch.empty((2, 20, 28), dtype=torch.uint8, device="cuda")), dict(peak=1023, gt=gt[:1])):
        with pytest.raises(ValueError):
            Kn.chroma_up4(src, **bad)
    with pytest.raises(ValueError):
        Kn.chroma_up4(torch.zeros((2, 5, 7), dtype=torch.uint8, device="cuda"), peak=1023)   # 8-bit planes have the peak 255
    flat = _dev(np.zeros(2 * 20 * 28 + 8, np.uint16))
    with pytest.raises(CdfoError, match="misaligned"):                                # destination off a 16-byte boundary
        Kn.chroma_up4(src, dst=flat[2:2 + 2 * 20 * 28].view(2, 20, 28), peak=1023)
    dst = _dev(np.zeros((2, 20, 28), np.uint16))
    nb = C.c_int(0)
    lib, vp, st = _lib.lib(), Kn._vp, Kn._stream()
    none = (None, 0, C.c_longlong(0), 0, 0, 0, None, 0, C.byref(nb), st)
    assert lib.cdfo_chroma_up4_u16(vp(src), 1 << 20, C.c_longlong(0), 1, 4096, 32, vp(dst), 1023, *none) == -1     # rows * pitch = 2^32
    assert lib.cdfo_chroma_up4_u16(vp(src), 16384, C.c_longlong(0), 1, 16384, 16384, vp(dst), 1023, *none) == -1   # 16 h w = 2^32
    assert lib.cdfo_chroma_up4_u16(vp(src), 6, C.c_longlong(0), 1, 5, 7, vp(dst), 1023, *none) == -1               # pitch < w
    assert lib.cdfo_chroma_up4_u16(vp(src), 7, C.c_longlong(35), 1, 5, 7, vp(dst), 0, *none) == -1                 # peak 0
    assert lib.cdfo_chroma_up4_u16(vp(src), 7, C.c_longlong(35), 1, 5, 7, vp(dst), 65536, *none) == -1
    torch.cuda.synchronize()
