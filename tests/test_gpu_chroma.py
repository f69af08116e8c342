"""cdfo_chroma_up4 (chroma.hip): the x4 chroma filter bit for bit against its numpy statement (tests/chroma_ref.py), its integer sum of
squared differences against numpy int64, and its argument checks.  A workgroup's tile is 32 x 16 source pixels."""
import ctypes as C

import numpy as np
import pytest
import torch

from chroma_ref import contents, up4, up4_sums

pytestmark = pytest.mark.gpu
# (h, w): 1x1 (every tap clamped), 1x5 and 5x1, 2x3, 5x7, 17x33 (one pixel more than a tile each way: halo across tile edges,
# four workgroups), 9x17
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 3), (5, 7), (17, 33), (9, 17)]


def _device_planes(p, pitched):
    """p uint8 [N,h,w] -> the same planes on the device: a dense stack, or a view whose pitch and plane stride exceed the plane, with
    255 everywhere outside the planes (which must never be read into the result)."""
    if not pitched:
        return torch.from_numpy(p).cuda()
    N, h, w = p.shape
    full = torch.full((N, h + 3, w + 5), 255, dtype=torch.uint8, device="cuda")
    view = full[:, 1:1 + h, 2:2 + w]
    view.copy_(torch.from_numpy(p))
    assert not view.is_contiguous() and view.stride(1) == w + 5 and view.stride(0) == (h + 3) * (w + 5)
    return view


@pytest.mark.parametrize("N,pitched", [(1, False), (2, True), (6, False), (6, True)])
@pytest.mark.parametrize("h,w", SHAPES)
def test_chroma_up4_bit_exact(h, w, N, pitched):
    from cdfo_amd import kernels as Kn
    for name, p in contents((N, h, w), 1000 * h + 10 * w + N).items():
        want = up4(p)
        if name != "random" and min(h, w) >= 5:          # the sums leave [0, 255] on both sides: both clamps are in the expectation
            s = (up4_sums(p) + 8192) >> 14
            assert s.min() < 0 and s.max() > 255 and want.min() == 0 and want.max() == 255
        out, sse = Kn.chroma_up4(_device_planes(p, pitched))
        assert sse is None and out.dtype == torch.uint8 and tuple(out.shape) == (N, 4 * h, 4 * w) and out.is_contiguous()
        assert torch.equal(out.cpu(), torch.from_numpy(want)), (name, np.argwhere(out.cpu().numpy() != want)[:5])
    # a destination of the caller's, filled in place; a single plane [h,w] is taken too
    dst = torch.full((N, 4 * h, 4 * w), 7, dtype=torch.uint8, device="cuda")
    got, _ = Kn.chroma_up4(_device_planes(p, pitched), dst=dst)
    assert got is dst and torch.equal(dst.cpu(), torch.from_numpy(want))
    one, _ = Kn.chroma_up4(_device_planes(p, pitched)[0])
    assert tuple(one.shape) == (1, 4 * h, 4 * w) and torch.equal(one.cpu()[0], torch.from_numpy(want[0]))


def _sse(out, gt, crop):
    hm, wm = min(out.shape[1], gt.shape[1]), min(out.shape[2], gt.shape[2])
    d = out[:, crop:hm - crop, crop:wm - crop].astype(np.int64) - gt[:, crop:hm - crop, crop:wm - crop].astype(np.int64)
    return (d * d).sum(axis=(1, 2))


@pytest.mark.parametrize("crop", [0, 2])
@pytest.mark.parametrize("dh,dw", [(0, 0), (2, 3), (-2, -4), (2, -4), (-3, 1)])
@pytest.mark.parametrize("N,h,w", [(2, 5, 7), (3, 17, 33)])
def test_chroma_up4_sse_is_the_exact_integer_sum(N, h, w, dh, dw, crop):
    """Ground truth of the output's size, larger, smaller and one of each; a dense stack (read in words where its rows are aligned)
    and a view of wider frames with an odd pitch (read in bytes); the source dense and pitched."""
    from cdfo_amd import kernels as Kn
    p = contents((N, h, w), 31 * h + dh - dw + crop)["random"]
    want = up4(p)
    Hg, Wg = 4 * h + dh, 4 * w + dw
    wide = np.random.RandomState(5 + h + dh - dw + crop).randint(0, 256, (N, Hg, Wg + 3 + Wg % 2)).astype(np.uint8)
    assert wide.shape[2] % 2 == 1                                            # an odd pitch
    cases = [(np.ascontiguousarray(wide[:, :, :Wg]), None), (wide[:, :, 3:3 + Wg], torch.from_numpy(wide).cuda()[:, :, 3:3 + Wg])]
    if Wg % 4 == 0:                                                          # words again, with rows longer than the frame
        wide4 = np.random.RandomState(6 + h).randint(0, 256, (N, Hg, Wg + 4)).astype(np.uint8)
        cases.append((wide4[:, :, :Wg], torch.from_numpy(wide4).cuda()[:, :, :Wg]))
    for gt, gd in cases:
        gd = torch.from_numpy(gt).cuda() if gd is None else gd
        ref = _sse(want, gt, crop)
        assert ref.min() > 0
        for pitched in (False, True):
            out, sse = Kn.chroma_up4(_device_planes(p, pitched), gt=gd, crop=crop)
            assert sse.dtype == torch.int64 and tuple(sse.shape) == (N,)
            assert np.array_equal(sse.cpu().numpy(), ref), (sse.cpu().numpy(), ref)
            assert torch.equal(out.cpu(), torch.from_numpy(want))


def test_chroma_up4_sse_of_a_region_of_one_pixel_and_of_equal_planes():
    from cdfo_amd import kernels as Kn
    p = np.array([[[200]], [[13]]], dtype=np.uint8)                          # 1x1 -> flat 4x4 planes of 200 and of 13
    gt = np.arange(18, dtype=np.uint8).reshape(2, 3, 3) * 3                  # common 3x3, crop 1: the pixel (1,1) alone, 12 and 39
    out, sse = Kn.chroma_up4(torch.from_numpy(p).cuda(), gt=torch.from_numpy(gt).cuda(), crop=1)
    assert sse.cpu().tolist() == [(200 - 12) ** 2, (13 - 39) ** 2]
    assert torch.equal(out.cpu(), torch.from_numpy(up4(p)))
    q = contents((2, 9, 17), 3)["binary"]
    out, sse = Kn.chroma_up4(torch.from_numpy(q).cuda(), gt=torch.from_numpy(up4(q)).cuda(), crop=0)
    assert sse.cpu().tolist() == [0, 0]
    worst = np.where(up4(q) >= 128, 0, 255).astype(np.uint8)                 # the largest sum the planes allow stays exact
    out, sse = Kn.chroma_up4(torch.from_numpy(q).cuda(), gt=torch.from_numpy(worst).cuda(), crop=0)
    assert np.array_equal(sse.cpu().numpy(), _sse(up4(q), worst, 0))


def test_bad_arguments_raise():
    from cdfo_amd import _lib
    from cdfo_amd import kernels as Kn
    from cdfo_amd._lib import CdfoError
    src = torch.zeros((2, 5, 7), dtype=torch.uint8, device="cuda")
    gt = torch.zeros((2, 6, 28), dtype=torch.uint8, device="cuda")
    with pytest.raises(CdfoError, match="invalid argument"):                          # crop leaves nothing of Hm = min(20, 6)
        Kn.chroma_up4(src, gt=gt, crop=3)
    Kn.chroma_up4(src, gt=gt, crop=2)
    with pytest.raises(CdfoError, match="invalid argument"):
        Kn.chroma_up4(src, gt=gt, crop=-1)
    with pytest.raises(ValueError):
        Kn.chroma_up4(src.cpu())                                                      # CPU tensors
    with pytest.raises(ValueError):
        Kn.chroma_up4(src, gt=gt.cpu())
    with pytest.raises(ValueError):
        Kn.chroma_up4(src.float())                                                    # wrong dtype
    with pytest.raises(ValueError):
        Kn.chroma_up4(src, gt=gt.to(torch.int8))
    with pytest.raises(ValueError):
        Kn.chroma_up4(src, gt=gt[:1])                                                 # one plane of ground truth for two planes
    with pytest.raises(ValueError):
        Kn.chroma_up4(src, dst=torch.empty((2, 20, 27), dtype=torch.uint8, device="cuda"))   # dst of the wrong shape
    with pytest.raises(ValueError):
        Kn.chroma_up4(src, dst=torch.empty((2, 20, 28), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        Kn.chroma_up4(src.transpose(1, 2))                                            # rows not contiguous
    flat = torch.empty(2 * 20 * 28 + 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(CdfoError, match="misaligned"):                                # destination off a 4-byte boundary
        Kn.chroma_up4(src, dst=flat[2:2 + 2 * 20 * 28].view(2, 20, 28))
    # a plane beyond the 32-bit offsets: refused from the arguments alone, before anything is launched
    dst = torch.empty((2, 20, 28), dtype=torch.uint8, device="cuda")
    nb = C.c_int(0)
    lib, vp, st = _lib.lib(), Kn._vp, Kn._stream()
    none = (None, 0, C.c_longlong(0), 0, 0, 0, None, 0, C.byref(nb), st)
    assert lib.cdfo_chroma_up4(vp(src), 1 << 20, C.c_longlong(0), 1, 4096, 32, vp(dst), *none) == -1       # rows * pitch = 2^32
    assert lib.cdfo_chroma_up4(vp(src), 16384, C.c_longlong(0), 1, 16384, 16384, vp(dst), *none) == -1     # 16 h w = 2^32
    assert lib.cdfo_chroma_up4(vp(src), 6, C.c_longlong(0), 1, 5, 7, vp(dst), *none) == -1                 # pitch < w
    assert lib.cdfo_chroma_up4(vp(src), 7, C.c_longlong(35), 0, 5, 7, vp(dst), *none) == -1                # no planes
    torch.cuda.synchronize()
